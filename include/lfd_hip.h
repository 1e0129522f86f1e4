/*
 * include/lfd_hip.h -- C ABI of liblfd_hip.so: the MI355X (gfx950) implementation of the
 * LFD dense-prediction hot path (post-processing, losses, conv stack).
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer is a DEVICE pointer unless its name ends in _host;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it, no hidden sync, no
 *     allocation: outputs and workspace are caller-owned (`*_workspace_bytes()` query);
 *   - return value: 0 (LFD_OK) or a negative lfd_status code; no C++ exception crosses the ABI;
 *   - thread-safe and re-entrant per stream.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference repository root).
 */
#ifndef LFD_HIP_H_
#define LFD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: lfd_head_level_ptrs_t grew (w{1,2}_folded, tower1_out, w{1,2}_perm), lfd_conv3x3_c64_chain_nhwc_f16 removed,
 * lfd_p32_* (fp32-storage precision mode) added.
 * 3: lfd_pl_* added (the same precision mode on hi/lo fp16 planes, csrc/planes.hip).
 * Every loader checks lfd_hip_abi_version() against this number. */
#define LFD_HIP_ABI_VERSION 3
#define LFD_MAX_LEVELS 8

/* Conventions of every entry point below.
 *  - Plain pointers and sizes; device pointers unless a parameter says "host".  Outputs and workspaces are caller-allocated
 *    (`*_workspace_bytes()` queries); nothing is allocated, freed or retained by the library between calls.
 *  - Every launch goes to the `lfd_stream_t` (= hipStream_t, NULL = the default stream) the caller passes; no entry point
 *    synchronises the device or the stream unless its comment says so.  Calls are re-entrant per stream; two streams must not
 *    share a workspace.
 *  - NHWC fp16 tensors are contiguous and 16-byte aligned (the kernels move them as 16-byte vectors and LDS-DMA lines); the
 *    fused-block, downsample-block, stride-2 data-gradient, conv + statistics and head-output entry points check it.
 *  - The return value is an `lfd_status`: 0 = launched, negative = refused before anything touched the device (argument
 *    checks run on the host).  No C++ types or exceptions cross the ABI. */
typedef void* lfd_stream_t; /* hipStream_t */

#if defined(LFD_BUILDING)
#define LFD_API __attribute__((visibility("default")))
#else
#define LFD_API
#endif

enum lfd_status {
  LFD_OK = 0,
  LFD_ERR_INVALID_ARGUMENT = -1,
  LFD_ERR_WORKSPACE_TOO_SMALL = -2,
  LFD_ERR_LAUNCH_FAILED = -3,
  LFD_ERR_UNSUPPORTED = -4,
  LFD_ERR_NO_DEVICE = -5
};

enum lfd_dtype { LFD_F32 = 0, LFD_F16 = 1 };

LFD_API int lfd_hip_abi_version(void);
LFD_API const char* lfd_hip_status_string(int status);
/* "gfx950;<compiler>;<build date>" */
LFD_API const char* lfd_hip_build_info(void);

/* Tuning knobs: which kernel variant an entry point dispatches to where several compute the SAME result (bit for bit; the
 * hash-identity tests flip them) or an A/B timing needs a choice.  Process-global, explicit, thread-safe (relaxed atomics);
 * the library reads no environment variable.  (Rounds 1-3 read LFD_* variables once per process inside the library; the
 * Python host layer still translates those names into lfd_tuning_set calls when it loads the library, lfd_amd/_lib.py.)
 * lfd_tuning_set -> 0 / LFD_ERR_INVALID_ARGUMENT; lfd_tuning_get of an unknown key -> 0. */
typedef enum lfd_tune_key {
  LFD_TUNE_HEAD2 = 0,          /* 1: wave-per-32-pixel head passes (k_head2); 0: k_head (4 waves per 64-pixel tile)        default 1 */
  LFD_TUNE_H2_CHUNK = 1,       /* >= 2 (even): force this many 32-pixel groups per k_head2 work chunk; 0: planned by size   default 0 */
  LFD_TUNE_H2_AGPR = 2,        /* 1: output pass loads the folded tower filters straight into AccVGPRs                     default 1 */
  LFD_TUNE_H2_A1 = 3,          /* 1: output pass reads the tower-1 activations pass 2 stored instead of recomputing them   default 1 */
  LFD_TUNE_STEM2X = 4,         /* 1: fused 'faster' stem with both 32-channel slabs per wave (k_stem2x)                    default 1 */
  LFD_TUNE_X2_ALN = 5,         /* 1: aligned dword frame loads + funnel shift in k_stem2x                                  default 1 */
  LFD_TUNE_X2_STAGGER = 6,     /* 1: start-up stagger of k_stem2x workgroups (measured slower since round 2)               default 0 */
  LFD_TUNE_BLOCK_ROWS = 7,     /* -1: residual block kernel by map size; 0: k_block64 (8 x 16 tiles); 1: k_block64_rows    default -1 */
  LFD_TUNE_ROWS_WGS = 8,       /* > 0: workgroups per k_block64_rows launch; 0: one per CU                                 default 0 */
  LFD_TUNE_CONV128_SPLITK = 9, /* 1: split-K kernel for 128 -> 128 3x3 convs on maps of <= 16384 pixels                    default 1 */
  LFD_TUNE_CONV0_VALU = 10,    /* 1: the first stem conv of the training path on the VALU kernels instead of MFMA         default 0 */
  LFD_TUNE_PL_C3 = 11,         /* planes mode, 3x3 s1 64-channel convs: 2 = k_pl_c3p (K split over a wave pair per SIMD),
                                  1 = k_pl_c3 (one wave per SIMD, epilogue under the next contraction), 0 = generic      default 2 */
  LFD_TUNE_PL_HEAD_OUT_REGS = 12, /* 1: lfd_pl_head_levels mode 2 with the fp32 tile landing in registers (k_pl_head_out)           default 1 */
  LFD_TUNE_PL_HEAD_ROLES = 13,  /* 1: lfd_pl_head_levels mode 1 with producer / consumer waves (k_pl_head_b2)                              default 1 */
  LFD_TUNE_PL_STEM = 14,        /* lfd_pl_stem2x on aligned fp16 frames: 0 = tiles, one wave per SIMD (k_pl_stem2x); 1 = row stream with producer
                                   and consumer waves (k_pl_stem2xs)                                                          default 1 */
  LFD_TUNE_COUNT = 15
} lfd_tune_key_t;
LFD_API int lfd_tuning_set(int32_t key, int32_t value);
LFD_API int32_t lfd_tuning_get(int32_t key);

/* HOST-side members of the nms_ext surface, for CPU tensors / numpy arrays (host pointers, no stream): the reference's
 * module dispatches `nms` on the tensor's device (nms_ext.cpp:18-27 -> cpu/nms_cpu.cpp:7-66) and has `soft_nms`
 * (nms_cpu.cpp:76-206) and `nms_match` (:220-283) for CPU tensors only.  Not a fallback of the device path.
 *   lfd_nms_cpu_f32:       keep[<= n] original indices, score-descending (ties: input order); suppress when IoU > thr
 *   lfd_soft_nms_cpu_f32:  method 1 linear / 2 gaussian / else hard; out[<= n][6] = x1,y1,x2,y2,score,index(as float)
 *   lfd_nms_match_cpu_f32: members[n] grouped (kept box first, then the boxes it matched with IoU >= thr), group_sizes[<= n] */
LFD_API int lfd_nms_cpu_f32(const float* dets, int64_t n, float iou_thr, int64_t* keep, int64_t* num_keep);
LFD_API int lfd_soft_nms_cpu_f32(const float* dets, int64_t n, float iou_thr, int32_t method, float sigma, float min_score,
                                 float* out, int64_t* num_out);
LFD_API int lfd_nms_match_cpu_f32(const float* dets, int64_t n, float iou_thr, int32_t* members, int32_t* group_sizes,
                                  int64_t* num_groups);
/* the same three on float64 data: the reference dispatches on the tensor's dtype (AT_DISPATCH_FLOATING_TYPES,
 * nms_cpu.cpp:70,212,287) and evaluates double tensors -- a numpy array's default dtype -- in double */
LFD_API int lfd_nms_cpu_f64(const double* dets, int64_t n, float iou_thr, int64_t* keep, int64_t* num_keep);
LFD_API int lfd_soft_nms_cpu_f64(const double* dets, int64_t n, float iou_thr, int32_t method, float sigma, float min_score,
                                 double* out, int64_t* num_out);
LFD_API int lfd_nms_match_cpu_f64(const double* dets, int64_t n, float iou_thr, int32_t* members, int32_t* group_sizes,
                                  int64_t* num_groups);

/* ------------------------------------------------------------------------------------------
 * NMS.  Replaces nms_ext.nms(dets[n,5] f32, thr) -> LongTensor[k]
 *   (lfd/model/utils/build/nms/src/nms_ext.cpp:18-27,45-49; CUDA path
 *    src/cuda/nms_kernel.cu:24-68 kernel + :71-138 host sort / D2H mask / serial scan;
 *    CPU path src/cpu/nms_cpu.cpp:7-66).
 * dets = {x1,y1,x2,y2,score}; IoU = inter/(Sa+Sb-inter) in fp32, no +1, strict `>`;
 * keep[0..*num_keep) = ORIGINAL row indices of the kept boxes in score-descending order
 * (ties: lower original index first -- the reference leaves tie order unspecified).
 * Sort, 64x64-tile bitmask and the greedy scan all run on the device (no D2H of the mask).
 */
LFD_API size_t lfd_nms_workspace_bytes(int64_t n);
LFD_API int lfd_nms_f32(const float* dets, int64_t n, float iou_thr, int64_t* keep /*[n]*/,
                int32_t* num_keep /*[1]*/, void* workspace, size_t workspace_bytes,
                lfd_stream_t stream);

/* batched_nms(bboxes[k,4], scores[k], inds[k], nms_cfg, class_agnostic)
 *   (lfd/model/utils/nms.py:119-158): per-class NMS through the coordinate-offset trick
 *   off = label * (max(bboxes)+1) evaluated in fp32 exactly as the reference does (:148-150),
 *   IoU decided on the shifted boxes, offset subtracted from the kept rows (:156).
 * out_dets[r] = {x1,y1,x2,y2,score} of kept row r, keep[r] = its index into the inputs. */
LFD_API size_t lfd_batched_nms_workspace_bytes(int64_t k);
LFD_API int lfd_batched_nms_f32(const float* boxes /*[k,4]*/, const float* scores /*[k]*/,
                        const int64_t* labels /*[k]*/, int64_t k, float iou_thr,
                        int32_t class_agnostic, float* out_dets /*[k,5]*/,
                        int64_t* keep /*[k]*/, int32_t* num_keep /*[1]*/, void* workspace,
                        size_t workspace_bytes, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused per-location decode + score threshold + multi-class NMS for a whole batch.
 * Replaces LFD.get_results / _get_results_for_single_image / predict_for_single_image's
 * post-processing (lfd/model/lfd.py:397-509, :577-655), distance2bbox (:261-282) and
 * multiclass_nms (lfd/model/utils/nms.py:161-220), for every image of the batch in one call.
 */
typedef struct lfd_detect_desc {
  int32_t num_levels;
  int32_t level_h[LFD_MAX_LEVELS];       /* head_indexes_to_feature_map_sizes (lfd.py:532) */
  int32_t level_w[LFD_MAX_LEVELS];
  int32_t level_stride[LFD_MAX_LEVELS];  /* point_strides: x=j*stride, y=i*stride (lfd.py:93-98) */
  float level_range_lo[LFD_MAX_LEVELS];  /* regression_ranges[i] */
  float level_range_hi[LFD_MAX_LEVELS];
  int32_t num_classes;                   /* C (foreground classes) */
  int32_t num_cls_channels;              /* C for sigmoid scores, C+1 for softmax (CE loss) */
  int32_t score_mode;                    /* 0: sigmoid (lfd.py:454); 1: softmax, drop last (:450-452) */
  int32_t decode_mode;                   /* 0: sigmoid(reg)*max(range) (:483-486); 1: exp(reg) (:480-482);
                                            2: reg*range_hi ('independent', :468-478);
                                            3: reg is the distance itself (FCOS, fcos.py:392 on fcos_head.py:145-146) */
  int32_t class_agnostic;                /* nms_cfg['class_agnostic'] (nms.py:143) */
  int32_t max_candidates;                /* capacity K_cap per image of candidate / output rows */
  float score_thr;                       /* strict `>` (nms.py:204) */
  float iou_thr;                         /* strict `>` (nms_cpu.cpp:62) */
} lfd_detect_desc_t;

LFD_API size_t lfd_detect_workspace_bytes(const lfd_detect_desc_t* desc, int32_t batch);
/* cls [N,P,C'] and reg [N,P,4] in `in_dtype` (level-concatenated, row-major as LFD.forward
 * returns them, lfd.py:526-542).  img_meta [N,3] f32 = {clamp_width, clamp_height,
 * resize_scale} (meta['resized_width'|'resized_height'|'resize_scale'], lfd.py:443-444,499).
 * Outputs (rows beyond the count are untouched):
 *   out_dets   [N,K_cap,5] f32  x1,y1,x2,y2,score of kept boxes, score-descending
 *   out_labels [N,K_cap]   i32  0-based class
 *   out_cand   [N,K_cap]   i32  candidate ordinal (position in the reference's nonzero() order)
 *   out_point  [N,K_cap]   i32  flat point index p of the kept box
 *   out_counts [N,4]       i32  {num_candidates (clamped), num_kept, overflow_flag, true_candidates}
 */
LFD_API int lfd_detect_batched(const lfd_detect_desc_t* desc, int32_t batch, const void* cls,
                       const void* reg, int32_t in_dtype, const float* img_meta,
                       float* out_dets, int32_t* out_labels, int32_t* out_cand,
                       int32_t* out_point, int32_t* out_counts, void* workspace,
                       size_t workspace_bytes, lfd_stream_t stream);

/* The same step for the sibling meta-architectures that share the multiclass_nms boundary:
 *   FCOS._get_results_for_single_image  (lfd/model/fcos.py:356-412)
 *   LFDv2._get_results_for_single_image (lfd/model/lfdv2.py:593-669)
 * which use its two arguments LFD leaves at their defaults, plus a per-level pre-selection:
 *   centerness  [N,P] logits or NULL: every class score is multiplied by sigmoid(centerness) -- multiclass_nms's
 *               score_factors (nms.py:192-193; fcos.py:376,403-409), applied BEFORE the threshold as there;
 *   pre_nms_limit  > 0: a level with more points keeps its pre_nms_limit best, ranked by the point's largest final score
 *               (fcos.py:383-390 ranks after the centerness factor; lfdv2.py:620-627), before decode and threshold.
 *               torch.topk leaves the choice among EQUAL keys open; this implementation takes the lowest point index;
 *   post_nms_limit > 0: multiclass_nms max_num (nms.py:217-219) -- out_counts[n][1] = min(kept, post_nms_limit), rows
 *               beyond it are unspecified.
 * Candidate order (out_cand) is point-major within the image, not the reference's "top-k order within the level": it
 * only reaches the results through the order of exactly equal scores, which the reference leaves unspecified.
 * Everything else -- outputs, img_meta, thresholds -- as lfd_detect_batched; workspace: lfd_detect_ex_workspace_bytes. */
typedef struct lfd_detect_ext {
  int32_t pre_nms_limit;
  int32_t post_nms_limit;
} lfd_detect_ext_t;
LFD_API size_t lfd_detect_ex_workspace_bytes(const lfd_detect_desc_t* desc, int32_t batch);
LFD_API int lfd_detect_batched_ex(const lfd_detect_desc_t* desc, const lfd_detect_ext_t* ext, int32_t batch,
                                  const void* cls, const void* reg, const void* centerness, int32_t in_dtype,
                                  const float* img_meta, float* out_dets, int32_t* out_labels, int32_t* out_cand,
                                  int32_t* out_point, int32_t* out_counts, void* workspace, size_t workspace_bytes,
                                  lfd_stream_t stream);

/* Second half of lfd_detect_batched for a workspace whose candidate arrays were filled by a producer kernel
 * (lfd_head_forward_decode_f16: the head's last pass thresholds, decodes and appends by itself): sort + suppression mask
 * + scan, 3 launches.  Candidates may have arrived in any order -- ties are broken by (point, class), the reference's
 * nonzero() order -- so out_dets / out_labels / out_point / out_counts equal lfd_detect_batched's; out_cand is the
 * arrival slot (not reproducible).  With more than max_candidates candidates (overflow flag) the retained subset is
 * arbitrary where lfd_detect_batched keeps the first K_cap in point order.
 * The workspace's two counter arrays must be zero before the first producer launch (lfd_detect_workspace_reset, once
 * per allocation); lfd_detect_from_candidates re-arms them. */
LFD_API int lfd_detect_workspace_reset(const lfd_detect_desc_t* desc, int32_t batch, void* workspace,
                                       size_t workspace_bytes, lfd_stream_t stream);
LFD_API int lfd_detect_from_candidates(const lfd_detect_desc_t* desc, int32_t batch, float* out_dets, int32_t* out_labels,
                                       int32_t* out_cand, int32_t* out_point, int32_t* out_counts, void* workspace,
                                       size_t workspace_bytes, lfd_stream_t stream);

/* Decode only (no threshold/NMS): boxes [N,P,4] f32 and scores [N,P,C] f32 for parity tests
 * and for callers that want the reference's intermediate tensors (lfd.py:449-499). */
LFD_API int lfd_decode_all(const lfd_detect_desc_t* desc, int32_t batch, const void* cls, const void* reg,
                   int32_t in_dtype, const float* img_meta, float* out_boxes, float* out_scores,
                   lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sigmoid focal loss.  Replaces sigmoid_focal_loss_ext.forward / .backward
 *   (lfd/model/losses/build/sigmoid_focal_loss/src/sigmoid_focal_loss_ext.cpp:19-57,
 *    src/cuda/sigmoid_focal_loss_cuda.cu:24-59 fwd, :62-97 bwd).
 * logits [n,c], targets [n] int64 (c == background, <0 == ignore), losses / d_logits [n,c]. */
LFD_API int lfd_sigmoid_focal_loss_fwd(const void* logits, const int64_t* targets, int64_t n, int32_t c,
                               float gamma, float alpha, void* losses, int32_t dtype,
                               lfd_stream_t stream);
LFD_API int lfd_sigmoid_focal_loss_bwd(const void* logits, const int64_t* targets, const void* d_losses,
                               int64_t n, int32_t c, float gamma, float alpha, void* d_logits,
                               int32_t dtype, lfd_stream_t stream);
/* Fused forward + sum reduction (weight_reduce_loss 'sum/avg_factor',
 * lfd/model/losses/utils.py:28-54): *loss_sum += sum(losses) accumulated in fp64 partials,
 * deterministic (fixed-order two-stage reduction).  workspace: lfd_reduce_workspace_bytes(). */
LFD_API size_t lfd_reduce_workspace_bytes(void);
LFD_API int lfd_sigmoid_focal_loss_sum_f32(const float* logits, const int64_t* targets, int64_t n, int32_t c,
                                   float gamma, float alpha, float* loss_sum /*[1]*/, void* workspace,
                                   size_t workspace_bytes, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * IoU loss on aligned xyxy boxes.  Replaces bbox_overlaps(is_aligned=True) + iou_loss
 *   (lfd/model/losses/iou_loss.py:67-79,98-102,105-123): loss = -log(max(ov/max(a1+a2-ov,1e-6), eps)).
 * bwd: d_pred[n,4] = d_loss[n] * dloss/dpred (autograd of the reference expression). */
LFD_API int lfd_iou_loss_fwd_f32(const float* pred, const float* target, int64_t n, float eps, float* loss,
                         lfd_stream_t stream);
LFD_API int lfd_iou_loss_bwd_f32(const float* pred, const float* target, const float* d_loss, int64_t n,
                         float eps, float* d_pred, lfd_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Target assignment: LFD.annotation_to_target / _generate_target_for_single_image
 *   (lfd/model/lfd.py:109-259; on the CPU with [P, G] broadcasts in the reference).
 * Whole batch in one launch.  Points are generated on the fly (lfd.py:84-107: x = j*stride, y = i*stride,
 * level-major, row-major).  Ground truth: gt_boxes [sumG,4] (x, y, w, h), gt_labels [sumG], image i owns rows
 * [gt_offsets[i], gt_offsets[i+1]).  Outputs: cls_targets [n, P, num_classes] (score in (0,1], 0 = negative,
 * -1 = gray / ignored), reg_targets [n, P, 4] (l, t, r, b deltas; divided by the level's upper range when
 * `independent`).  assign_mode: 0 'longer', 1 'shorter', 2 'sqrt', 3 'dist' (lfd.py:206-215).
 * fp32, reference expression order, IEEE divide / sqrt: decisions and regression targets identical to the
 * reference, scores identical up to the last bit of the host's sqrt routine. */
typedef struct {
  int32_t n, num_levels;
  int32_t level_h[LFD_MAX_LEVELS], level_w[LFD_MAX_LEVELS], stride[LFD_MAX_LEVELS];
  int32_t reg_lo[LFD_MAX_LEVELS], reg_hi[LFD_MAX_LEVELS];     /* regression_ranges (lfd.py:43) */
  int32_t gray_lo[LFD_MAX_LEVELS], gray_hi[LFD_MAX_LEVELS];   /* gray ranges (lfd.py:49-50) */
  int32_t total_points, num_classes;
  int32_t assign_mode, independent;
} lfd_assign_desc_t;
LFD_API int lfd_assign_targets_f32(const lfd_assign_desc_t* d, const float* gt_boxes, const int64_t* gt_labels,
                           const int32_t* gt_offsets, float* cls_targets, float* reg_targets, lfd_stream_t stream);

/* CrossEntropyLoss core (lfd/model/losses/cross_entropy_loss.py:12-50 -> F.cross_entropy(pred, label,
 * reduction='none'); TT100K configs): loss[i] = logsumexp(logits[i,:]) - logits[i, labels[i]];
 * bwd: d_logits[i,j] = d_loss[i] * (softmax(logits[i,:])[j] - [j == labels[i]]). */
LFD_API int lfd_cross_entropy_fwd_f32(const float* logits, const int64_t* labels, int64_t m, int32_t channels, float* loss,
                              lfd_stream_t stream);
LFD_API int lfd_cross_entropy_bwd_f32(const float* logits, const int64_t* labels, const float* d_loss, int64_t m,
                              int32_t channels, float* d_logits, lfd_stream_t stream);

/* GIoU / DIoU / CIoU losses of aligned box pairs (lfd/model/losses/iou_loss.py:127-169, :172-223, :226-283; the other
 * members of LFD's IoU-type regression-loss family, lfd.py:64-66): kind 1 | 2 | 3; loss[n] and -- when
 * d_loss_d_pred != NULL -- the gradient [n,4] w.r.t. the predicted xyxy box, obtained by forward-mode
 * differentiation of the reference expression inside the kernel (max / min / clamp route like autograd). */
LFD_API int lfd_box_loss_f32(const float* pred, const float* target, int64_t n, int32_t kind, float eps, float* loss,
                     float* d_loss_d_pred, lfd_stream_t stream);
/* The remaining classification losses LFD accepts (lfd.py:52-56).  lfd_bce_with_logits_f32: elementwise
 * F.binary_cross_entropy_with_logits(logits, targets, reduction='none') over n values (bce_with_logits_loss.py:28-44) and
 * its derivative sigmoid(x) - t.  lfd_quality_focal_loss_f32 (gfocal_loss.py:11-52): per row the sum over classes of
 * BCE(x, t) |t - sigmoid(x)|^beta with t = scores[row] at class labels[row] (if it is a foreground label) and 0 elsewhere;
 * d_logits [rows, channels] (nullable) = its derivative. */
LFD_API int lfd_bce_with_logits_f32(const float* logits, const float* targets, int64_t n, float* loss, float* d_logits,
                            lfd_stream_t stream);
LFD_API int lfd_quality_focal_loss_f32(const float* logits, const int64_t* labels, const float* scores, int64_t rows,
                               int32_t channels, float beta, float* loss, float* d_logits, lfd_stream_t stream);
/* LFD's "independent" regression losses (lfd.py:61-66), elementwise over n values: kind 1 smooth-L1 with `beta`
 * (lfd/model/losses/smooth_l1_loss.py:11-22), 2 L1 (:25-30), 3 MSE (mse_loss.py:11-13); loss[n] and, when
 * d_loss_d_pred != NULL, the derivative w.r.t. pred. */
LFD_API int lfd_pointwise_loss_f32(const float* pred, const float* target, int64_t n, int32_t kind, float beta, float* loss,
                           float* d_loss_d_pred, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused LFD.get_loss (lfd/model/lfd.py:284-395): replaces the boolean gathers (green rows :309-315, positive
 * rows :319-321), the label construction (:328), FocalLoss / CrossEntropyLoss + IoULoss on the gathered rows
 * (:333-384, decode of prediction and target :360-377) and the three `.item()` syncs (:389-395) by
 *   sums     : one pass over all N*P rows -> 8 doubles {cls_sum, reg_sum, n_pos, sum of positive scores,
 *              n_green, 0, 0, 0} (fp64 block partials + fixed-order second stage: deterministic);
 *   finalize : out[8] floats {classification_loss, regression_loss, loss, n_pos, avg_factor_cls,
 *              avg_factor_reg, n_green(local), rank_scale}; `global_sums` are the sums all-reduced over the
 *              image-parallel ranks (== local_sums on one GPU) because the reference normalises by the
 *              global-batch n_pos (executor.py:198-200); rank_scale = world size when gradients are
 *              averaged over ranks afterwards (1 otherwise);
 *   bwd      : dense d loss / d pred_cls [N,P,channels], d loss / d pred_reg [N,P,4] for upstream
 *              gradients grad_out[3] of {classification_loss, regression_loss, loss}.
 * pred_cls has num_classes channels for cls_loss 0 (sigmoid focal) and num_classes + 1 for cls_loss 1
 * (cross entropy, background = last channel).  No positives -> regression_loss 0 with zero gradient
 * (lfd.py:386-387).  All tensors fp32, contiguous.
 */
typedef struct lfd_loss_desc {
  int32_t n, num_levels;
  int32_t level_h[LFD_MAX_LEVELS], level_w[LFD_MAX_LEVELS], stride[LFD_MAX_LEVELS];
  float range_max[LFD_MAX_LEVELS];  /* max(regression_ranges[i]) ('sigmoid' decode, lfd.py:368-373) */
  int32_t total_points, num_classes;
  int32_t cls_loss;                 /* 0 FocalLoss (sigmoid), 1 CrossEntropyLoss */
  int32_t decode_mode;              /* 0 sigmoid * range_max, 1 exp (lfd.py:366-374) */
  float gamma, alpha, iou_eps;
  float cls_loss_weight, reg_loss_weight;   /* loss_weight of the two loss modules */
  int32_t cls_weighted, reg_weighted;       /* enable_classification_weight / enable_regression_weight */
} lfd_loss_desc_t;
LFD_API size_t lfd_get_loss_workspace_bytes(void);
LFD_API int lfd_get_loss_sums_f32(const lfd_loss_desc_t* d, const float* pred_cls, const float* pred_reg,
                          const float* cls_targets, const float* reg_targets, void* workspace, size_t workspace_bytes,
                          double* sums, lfd_stream_t stream);
LFD_API int lfd_get_loss_finalize_f32(const lfd_loss_desc_t* d, const double* local_sums, const double* global_sums,
                              float rank_scale, float* out, lfd_stream_t stream);
LFD_API int lfd_get_loss_bwd_f32(const lfd_loss_desc_t* d, const float* pred_cls, const float* pred_reg,
                         const float* cls_targets, const float* reg_targets, const float* finalized,
                         const float* grad_out, float* grad_cls, float* grad_reg, lfd_stream_t stream);

/* Fused get_loss for every pair of loss modules LFD / LFDv2 accept (csrc/getloss_ex.hip): the three stages, the sums[8] and
 * out[8] layouts, the row classification and the normalisers of lfd_get_loss_* above, with
 *   cls_loss 0 FocalLoss (sigmoid), 1 CrossEntropyLoss (num_classes + 1 channels), 2 QualityFocalLoss
 *            (gfocal_loss.py:11-51: per class B(x, t) |t - sigmoid(x)|^qfl_beta, t = the row's maximum score at the label's
 *            channel of a positive row and 0 elsewhere, a constant of the backward), 3 BCEWithLogitsLoss (lfd.py:342-347:
 *            B(x_c, target_c) against the row's whole soft target vector, summed);
 *   reg_loss 0 IoULoss, 1 GIoULoss, 2 DIoULoss, 3 CIoULoss (iou_loss.py:105-283) on distance2bbox of the decoded
 *            prediction and of the target, times the row's score when reg_weighted; 4 SmoothL1Loss(smooth_l1_beta),
 *            5 MSELoss (lfd.py:354-358, 'independent'): elementwise on the raw four outputs against the raw targets,
 *            summed over the four components, no decode; reg_weighted is LFD_ERR_UNSUPPORTED with these two.
 * Reduction 'mean' only.  lfd_get_loss_* keeps the Focal / CrossEntropy + IoU pair with its own kernels. */
typedef struct lfd_loss_ex_desc {
  int32_t n, num_levels;
  int32_t level_h[LFD_MAX_LEVELS], level_w[LFD_MAX_LEVELS], stride[LFD_MAX_LEVELS];
  float range_max[LFD_MAX_LEVELS];  /* max(regression_ranges[i]) ('sigmoid' decode, lfd.py:368-373) */
  int32_t total_points, num_classes;
  int32_t cls_loss;                 /* 0..3, see above */
  int32_t reg_loss;                 /* 0..5, see above */
  int32_t decode_mode;              /* 0 sigmoid * range_max, 1 exp (lfd.py:366-374); unused by reg_loss 4, 5 */
  float gamma, alpha;               /* FocalLoss */
  float qfl_beta;                   /* QualityFocalLoss */
  float smooth_l1_beta;             /* SmoothL1Loss (> 0) */
  float box_eps;                    /* eps of the IoU-family module */
  float cls_loss_weight, reg_loss_weight;   /* loss_weight of the two loss modules */
  int32_t cls_weighted, reg_weighted;       /* enable_classification_weight / enable_regression_weight */
} lfd_loss_ex_desc_t;
LFD_API size_t lfd_get_loss_ex_workspace_bytes(void);
LFD_API int lfd_get_loss_ex_sums_f32(const lfd_loss_ex_desc_t* d, const float* pred_cls, const float* pred_reg,
                             const float* cls_targets, const float* reg_targets, void* workspace, size_t workspace_bytes,
                             double* sums, lfd_stream_t stream);
LFD_API int lfd_get_loss_ex_finalize_f32(const lfd_loss_ex_desc_t* d, const double* local_sums, const double* global_sums,
                                 float rank_scale, float* out, lfd_stream_t stream);
LFD_API int lfd_get_loss_ex_bwd_f32(const lfd_loss_ex_desc_t* d, const float* pred_cls, const float* pred_reg,
                            const float* cls_targets, const float* reg_targets, const float* finalized,
                            const float* grad_out, float* grad_cls, float* grad_reg, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sibling meta-architectures: target assignment and fused get_loss on the device (csrc/assign_sibling.hip,
 * csrc/getloss_fcos.hip).  Conventions of lfd_assign_targets_f32: whole batch in one launch, one thread per (image,
 * point), points generated on the fly, gt_boxes [num_boxes,4] (x, y, w, h), gt_labels [num_boxes], image i owns rows
 * [gt_offsets[i], gt_offsets[i+1]) (device array of n + 1 values; rows outside [0, num_boxes) are never read).
 * gt_offsets_host (nullable) is the caller's host copy of gt_offsets: when given it is checked before the launch
 * (non-negative, non-decreasing, <= num_boxes) -- the device copy cannot be without a sync.  Any G per image (boxes are
 * staged through LDS in fixed-size chunks), G = 0 included.  fp32, reference expression order, IEEE divide / sqrt.
 *
 * lfd_assign_targets_fcos_f32: FCOS.annotation_to_target (lfd/model/fcos.py:108-209).  Per (point, box)
 *   dist = (px-x, py-y, (x+w-1)-px, (y+h-1)-py); the pair is valid iff min(dist) > 0 and range_lo <= max(dist) <=
 *   range_hi of the point's level (both inclusive; floats: the last level's bound is 1e8).  The point takes the valid
 *   box of smallest area w*h, ties -> lowest box index.  labels int64 [n,P] = that box's label or num_classes when no
 *   box is valid; reg_targets [n,P,4] = dist of the chosen box (box 0 when none is valid, zeros when the image has no
 *   box).  multi_label != 0 (FCOSv1, fcos.py:550-656): labels int64 [n,P,num_classes], 0 where a valid box of that
 *   class covers the point, 1 elsewhere; reg_targets unchanged.
 * lfd_assign_targets_v2_f32: LFDv2._generate_target_for_single_image (lfd/model/lfdv2.py:278-418) over
 *   lfd_assign_desc_t (integer ranges, assign_mode 0..3, independent).  score = sqrt(min(l,r)/max(l,r) *
 *   min(t,b)/max(t,b)) inside the box (hit test >= 0, denominators clamped at 0.01), 1 in the stride-sized core zone,
 *   times the linear relaxation across the gray band; cls_targets [n,P,C] = per-class maximum of the positive scores,
 *   reg_targets [n,P,4] = delta of the box with the largest score (/ reg_hi when independent), ties -- the all-zero row
 *   included -- -> lowest box index. */
typedef struct {
  int32_t n, num_levels;
  int32_t level_h[LFD_MAX_LEVELS], level_w[LFD_MAX_LEVELS], stride[LFD_MAX_LEVELS];
  float range_lo[LFD_MAX_LEVELS], range_hi[LFD_MAX_LEVELS];   /* regress_ranges (fcos.py:19) */
  int32_t total_points, num_classes;
  int32_t multi_label, reserved_;
} lfd_assign_fcos_desc_t;
LFD_API int lfd_assign_targets_fcos_f32(const lfd_assign_fcos_desc_t* d, const float* gt_boxes, const int64_t* gt_labels,
                                int64_t num_boxes, const int32_t* gt_offsets, const int32_t* gt_offsets_host,
                                int64_t* labels, float* reg_targets, lfd_stream_t stream);
LFD_API int lfd_assign_targets_v2_f32(const lfd_assign_desc_t* d, const float* gt_boxes, const int64_t* gt_labels,
                              int64_t num_boxes, const int32_t* gt_offsets, const int32_t* gt_offsets_host,
                              float* cls_targets, float* reg_targets, lfd_stream_t stream);

/* Fused FCOS.get_loss / FCOSv1.get_loss (lfd/model/fcos.py:240-317, :687-768), same three stages as lfd_get_loss_*:
 *   sums     : one pass over all N*P rows -> 8 doubles {cls_sum (sigmoid focal of every row; multi_label: the flattened
 *              one-class focal), reg_sum (box loss of distance2bbox(prediction) vs distance2bbox(target), weighted by
 *              the centerness target), ctr_sum (BCE-with-logits of the centerness logit), n_pos, sum of centerness
 *              targets, 0, 0, 0} over the positive rows (label != num_classes; any class present when multi_label);
 *              fp64 block partials + fixed-order second stage: deterministic;
 *   finalize : out[8] floats {classification_loss, regression_loss, centerness_loss, loss, n_pos, avg_factor_cls
 *              (= n_pos + N), avg_factor_reg (= sum of centerness targets), rank_scale}; global_sums = the sums
 *              all-reduced over image-parallel ranks (== local_sums on one GPU), N = n * rank_scale (the global batch
 *              of equally sized per-rank batches); no positive -> regression and centerness loss 0, zero gradient;
 *   bwd      : dense d/d pred_cls [N,P,C], d/d pred_reg [N,P,4], d/d pred_ctr [N,P,1] for upstream gradients
 *              grad_out[4] of {classification_loss, regression_loss, centerness_loss, loss}.
 * The centerness targets are constants (computed from the regression targets).  labels as written by
 * lfd_assign_targets_fcos_f32.  All float tensors fp32, contiguous. */
typedef struct {
  int32_t n, num_levels;
  int32_t level_h[LFD_MAX_LEVELS], level_w[LFD_MAX_LEVELS], stride[LFD_MAX_LEVELS];
  int32_t total_points, num_classes;
  int32_t multi_label;
  int32_t box_loss;                 /* 0 IoULoss, 1 GIoULoss, 2 DIoULoss, 3 CIoULoss (lfd/model/losses/iou_loss.py) */
  float gamma, alpha, box_eps;
  float cls_loss_weight, reg_loss_weight, ctr_loss_weight;   /* loss_weight of the three loss modules */
} lfd_fcos_loss_desc_t;
LFD_API size_t lfd_fcos_loss_workspace_bytes(void);
LFD_API int lfd_fcos_loss_sums_f32(const lfd_fcos_loss_desc_t* d, const float* pred_cls, const float* pred_reg,
                           const float* pred_ctr, const int64_t* labels, const float* reg_targets, void* workspace,
                           size_t workspace_bytes, double* sums, lfd_stream_t stream);
LFD_API int lfd_fcos_loss_finalize_f32(const lfd_fcos_loss_desc_t* d, const double* local_sums, const double* global_sums,
                               float rank_scale, float* out, lfd_stream_t stream);
LFD_API int lfd_fcos_loss_bwd_f32(const lfd_fcos_loss_desc_t* d, const float* pred_cls, const float* pred_reg,
                          const float* pred_ctr, const int64_t* labels, const float* reg_targets, const float* finalized,
                          const float* grad_out, float* grad_cls, float* grad_reg, float* grad_ctr, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Parameter update of a training iteration over one flat fp32 buffer (all tensors of a param group
 * contiguous, 16-byte aligned).  Replaces OptimizerHook.after_train_iter's
 *   clip_grad.clip_grad_norm_(params, max_norm, norm_type=2)   (lfd/execution/hooks/optimizer_hook.py:21-24,30-33)
 *   optimizer.step() with torch.optim.SGD(lr, momentum, weight_decay) (optimizer_hook.py:36, WIDERFACE_LFD_S.py:216-226)
 * lfd_grad_norm_clip_coef_f32: norm_and_coef[0] = ||grads||_2 (fp64 accumulation, deterministic),
 *   norm_and_coef[1] = min(max_norm / (norm + 1e-6), 1).  extra_sumsq (nullable, device) is added to the
 *   sum of squares before the root (several buffers sharing one norm); sumsq_out (nullable) receives the total.
 * lfd_sgd_step_f32: g *= coef (when apply_clip; written back when write_clipped_grads, as
 *   clip_grad_norm_ mutates .grad); d = g + wd * p; buf = first_step ? d : momentum * buf + (1 - dampening) * d;
 *   d = nesterov ? d + momentum * buf : buf; p -= lr * d   (torch/optim/sgd.py _single_tensor_sgd).
 *   Overflow guard of the fp16 activation-gradient path (csrc/train.hip stores dz as fp16 x loss scale): when
 *   norm_and_coef != NULL and norm_and_coef[0] -- the total gradient norm -- is not finite (an inf gradient gives
 *   norm = inf and coef = 0, and 0 * inf = NaN would be written into the weights; a NaN gradient gives NaN), the whole
 *   update is skipped: parameters, momentum and gradients untouched; the caller reads the norm and lowers its loss scale
 *   (lfd_amd.train.DynamicLossScale).  norm_and_coef must be given when apply_clip != 0.
 */
LFD_API size_t lfd_grad_norm_workspace_bytes(void);
LFD_API int lfd_grad_norm_clip_coef_f32(const float* grads, int64_t n, float max_norm, const double* extra_sumsq,
                                void* workspace, size_t workspace_bytes, float* norm_and_coef, double* sumsq_out,
                                lfd_stream_t stream);
/* grads *= norm_and_coef[1] (the in-place scaling of clip_grad_norm_ when the update is not fused with it) */
LFD_API int lfd_scale_by_clip_coef_f32(float* grads, int64_t n, const float* norm_and_coef, lfd_stream_t stream);
LFD_API int lfd_sgd_step_f32(float* params, float* grads, float* momentum_buf, int64_t n, float lr, float momentum,
                     float dampening, float weight_decay, int32_t nesterov, int32_t first_step,
                     const float* norm_and_coef, int32_t apply_clip, int32_t write_clipped_grads, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Inference conv stack, NHWC fp16, fp32 accumulate on MFMA.  Replaces the nn.Conv2d +
 * nn.BatchNorm2d (folded) + ReLU (+ residual add) units of LFDResNet
 *   (lfd/model/backbone/lfd_resnet.py:96-154 FasterBlock, :21-93 FastBlock, :157-215 FastestBlock,
 *    :354-439 stem, :458-468 downsample; executed by cuDNN in the reference).
 * out = relu?( conv(in, w) + bias (+ residual) ), optionally followed in the same kernel by a
 * chained 1x1 conv: out = relu?( conv1x1(relu?(conv(in,w)+bias), tail_w) + tail_bias ).
 * Weights are pre-packed in MFMA fragment order (see lfd_pack_conv_weight_f16).
 */
typedef struct lfd_conv_desc {
  int32_t n, h, w;      /* input dims (NHWC) */
  int32_t cin, cout;    /* cin in {32,64,128} with the cout values csrc/conv.hip lists; or, when either side is above 128
                         * (csrc/conv_wide.hip): cin a multiple of 64, cout a multiple of 32, both <= 512, no chained 1x1 */
  int32_t ks, stride;   /* 1|3 (pad = ks/2), 1|2 */
  int32_t relu;
  int32_t tail_cout;    /* 0: no chained 1x1; else must equal cout */
  int32_t tail_relu;
} lfd_conv_desc_t;

LFD_API size_t lfd_conv_packed_weight_halfs(int32_t cin, int32_t cout, int32_t ks);
/* First conv of a residual block together with its identity branch (lfd_resnet.py:458-468): the
 * conv3x3 stride 2 (+BN+ReLU) -> out and the downsample conv1x1 stride 2 (+BN, no ReLU) -> ds_out are
 * produced by ONE launch from the same input tile (the 1x1 s2 reads the 3x3's centre tap). */
LFD_API int lfd_conv2d_downsample_nhwc_f16(const lfd_conv_desc_t* desc, const void* in, void* out,
                                           const void* w_packed, const float* bias,
                                           const void* ds_w_packed, const float* ds_bias, void* ds_out,
                                           const void* zeros, lfd_stream_t stream);

/* The checks and the dispatch of lfd_conv2d_nhwc_f16 on a descriptor alone (no residual): 0 if the call would reach a kernel,
 * else LFD_ERR_UNSUPPORTED (LFD_ERR_INVALID_ARGUMENT for a malformed descriptor).  Launches nothing, needs no device. */
LFD_API int lfd_conv2d_nhwc_f16_supported(const lfd_conv_desc_t* desc);

LFD_API int lfd_conv2d_nhwc_f16(const lfd_conv_desc_t* desc, const void* in, void* out,
                                const void* w_packed, const float* bias, const void* residual,
                                const void* tail_w_packed, const float* tail_bias,
                                const void* zeros /* 4096-byte line: [0,2048) zero (read), [2048,4096) trash (written) */, lfd_stream_t stream);

/* A whole residual block of the backbone without downsample branch (FasterBlock, lfd_resnet.py:96-154; every block of a
 * stage but the first) in ONE launch:   out = relu( conv3x3(relu(conv3x3(in, w1) + b1), w2) + b2 + in ),  64 -> 64 -> 64
 * channels, stride 1, BN folded into (w, b), NHWC fp16 [n, h, w, 64].  The intermediate map lives in LDS tile by tile
 * (csrc/block.hip: producer / consumer wave specialisation, both filters register-stationary); results are bit-identical
 * to two lfd_conv2d_nhwc_f16 launches.  w1_packed / w2_packed: lfd_conv_packed_weight_halfs(64, 64, 3) halfs each;
 * `in` must not alias `out`; zeros: the 4096-byte line of lfd_conv2d_nhwc_f16. */
LFD_API int lfd_fasterblock_fused_f16(int32_t n, int32_t h, int32_t w, const void* in, void* out, const void* w1_packed,
                                      const float* b1, const void* w2_packed, const float* b2, const void* zeros,
                                      lfd_stream_t stream);

/* The same block at 128 channels on the SMALL maps of the last backbone stage (17 x 30 at 1080p; WIDERFACE_LFD_S.py:97-146,
 * lfd_resnet.py:96-154) in ONE launch:   out = relu( conv3x3(relu(conv3x3(in, w1) + b1), w2) + b2 + in ),  128 -> 128 -> 128,
 * NHWC fp16 [n, h, w, 128].  A workgroup owns 4 x 8 output pixels and recomputes the 6 x 10 halo of the intermediate map in
 * LDS; both filters are streamed from L2 per workgroup, so this form is for maps of a few thousand pixels per launch (the
 * caller decides; csrc/block128.hip).  Results are bit-identical to two lfd_conv2d_nhwc_f16 launches on their split-K path
 * (n * h * w <= 16384).  w1_packed / w2_packed: lfd_conv_packed_weight_halfs(128, 128, 3) halfs each; `in` must not alias
 * `out`; all pointers 16-byte aligned. */
LFD_API int lfd_fasterblock128_fused_f16(int32_t n, int32_t h, int32_t w, const void* in, void* out, const void* w1_packed,
                                         const float* b1, const void* w2_packed, const float* b2, lfd_stream_t stream);

/* The FIRST block of a backbone stage -- the FasterBlock with a downsample branch (lfd_resnet.py:96-154, branch :458-468) --
 * in ONE launch:   y1 = relu(conv3x3_s2(in, w1) + b1);  ident = conv1x1_s2(in, wd) + bd;
 *                  out = relu(conv3x3_s1(y1, w2) + b2 + ident),      64 -> 64 channels, BN folded, NHWC fp16,
 * in [n, h, w, 64] -> out [n, (h-1)/2+1, (w-1)/2+1, 64].  y1 and ident live in LDS row rings (csrc/down.hip: a workgroup
 * streams down a 30-column strip; producer / consumer waves, three register-stationary filters); results are bit-identical
 * to lfd_conv2d_downsample_nhwc_f16 followed by lfd_conv2d_nhwc_f16 with `residual`.  w1_packed / w2_packed:
 * lfd_conv_packed_weight_halfs(64, 64, 3) halfs, wd_packed: lfd_conv_packed_weight_halfs(64, 64, 1); `in` must not alias
 * `out`; zeros: the 4096-byte line of lfd_conv2d_nhwc_f16. */
LFD_API int lfd_downblock_fused_f16(int32_t n, int32_t h, int32_t w, const void* in, void* out, const void* w1_packed,
                                    const float* b1, const void* wd_packed, const float* bd, const void* w2_packed,
                                    const float* b2, const void* zeros, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise operators of the sibling necks / heads, NHWC fp16, channels a multiple of 8:
 *   lfd_upsample_nearest_add_nhwc_f16   dst[n,H,W,c] += nearest(src[n,h,w,c]) -- the merge step of FPN / SimpleFPN
 *                                       (`lateral[i-1] += nn.Upsample(size, mode='nearest')(lateral[i])`,
 *                                       lfd/model/neck/fpn.py:133-135, simple_fpn.py:147-157); source index =
 *                                       min(floorf(dst_index * float(in)/out), in-1) as ATen computes it; fp32 add.
 *   lfd_relu_inplace_f16                nn.ReLU(inplace=True) in front of an extra level: it rewrites the PREVIOUS
 *                                       output level as well (fpn.py:66-79, simple_fpn.py:84-99 feed fpn_outputs[-1]).
 *   lfd_maxpool3x3s2_nhwc_f16           extra_type='pooling': nn.MaxPool2d(3, 2, 1) (fpn.py:74) -> [n, (h+1)/2, (w+1)/2, c].
 *   lfd_pack_level_outputs_f32          channels c0 .. c0+count of a level's fp32 output-conv map [n, hw, src_channels]
 *                                       -> rows point_offset .. +hw of the level-concatenated [n, total_points, count]
 *                                       tensor the meta-architecture returns (fcos.py:426-449, lfdv2.py:683-702),
 *                                       times `scale` (the head's per-level Scale), op 1: then expf
 *                                       (fcos_head.py:145-146). */
LFD_API int lfd_upsample_nearest_add_nhwc_f16(void* dst, const void* src, int32_t n, int32_t H, int32_t W, int32_t h,
                                              int32_t w, int32_t c, lfd_stream_t stream);
LFD_API int lfd_relu_inplace_f16(void* x, int64_t count, lfd_stream_t stream);
LFD_API int lfd_maxpool3x3s2_nhwc_f16(const void* in, void* out, int32_t n, int32_t h, int32_t w, int32_t c,
                                      lfd_stream_t stream);
LFD_API int lfd_pack_level_outputs_f32(const float* src, float* dst, int32_t n, int32_t hw, int32_t src_channels, int32_t c0,
                                       int32_t count, int32_t total_points, int32_t point_offset, float scale, int32_t op,
                                       lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training pass of the FPN / SimpleFPN necks: the backward of the element-wise operators above and the bias gradient of a plain
 * conv (csrc/sibling_train.hip).  Gradients are NHWC fp16 carrying the loss scale; fp32 arithmetic, one rounding to fp16.  Every
 * kernel is a gather (no atomics): two runs give the same bits.  Nothing is launched when a status code is returned.
 *   lfd_upsample_nearest_add_bwd_nhwc_f16  replaces the autograd backward of `lateral[i-1] += nn.Upsample(size,
 *                                       mode='nearest')(lateral[i])` (lfd/model/neck/fpn.py:133-135, simple_fpn.py:147-157):
 *                                       g_src[n,yy,xx,:] += sum of g_dst[n,y,x,:] over the (y, x) whose forward source index
 *                                       min(floorf(y * float(h)/H), h-1) (same for x) is (yy, xx) -- the forward's expression
 *                                       evaluated per candidate.  g_src [n,h,w,c] in place, g_dst [n,H,W,c]; no aliasing.
 *   lfd_maxpool3x3s2_bwd_nhwc_f16       replaces the autograd backward of the extra_type='pooling' level, nn.MaxPool2d(3, 2, 1)
 *                                       (fpn.py:74, simple_fpn.py:92): g_in[n,y,x,:] (+= if accumulate) g_out of every window
 *                                       whose argmax is (y, x); x [n,h,w,c] is the forward input, the argmax is recomputed:
 *                                       the FIRST position in scan order that attains the maximum (ATen's strict `>` update).
 *   lfd_relu_bwd_add_f16                replaces the autograd backward of the nn.ReLU(inplace=True) in front of an extra level
 *                                       (fpn.py:66-79, simple_fpn.py:84-99), which rewrites the previous output level as well:
 *                                       out = (g_a + g_b) * [y > 0], g_b nullable; out may be g_a or g_b.
 *   lfd_bias_grad_nhwc_f16              replaces the autograd bias gradient of the nn.Conv2d(bias=True) laterals / output
 *                                       convs (fpn.py:57-82): dbias[c] += inv_scale * sum over rows of dy[row, c]; dy
 *                                       [rows, c] fp16, c in {32, 64, 128}; fp32 partial sums per block, fixed-order fp64
 *                                       final.  workspace: lfd_bias_grad_workspace_bytes(). */
LFD_API int lfd_upsample_nearest_add_bwd_nhwc_f16(void* g_src, const void* g_dst, int32_t n, int32_t H, int32_t W, int32_t h,
                                                  int32_t w, int32_t c, lfd_stream_t stream);
LFD_API int lfd_maxpool3x3s2_bwd_nhwc_f16(const void* x, const void* g_out, void* g_in, int32_t n, int32_t h, int32_t w,
                                          int32_t c, int32_t accumulate, lfd_stream_t stream);
LFD_API int lfd_relu_bwd_add_f16(const void* y, const void* g_a, const void* g_b, void* out, int64_t count, lfd_stream_t stream);
LFD_API size_t lfd_bias_grad_workspace_bytes(void);
LFD_API int lfd_bias_grad_nhwc_f16(const void* dy, int64_t rows, int32_t c, float inv_scale, float* dbias, void* workspace,
                                   size_t workspace_bytes, lfd_stream_t stream);

/* Parity instrument (not on the product path): the same MFMA conv kernels with the fp32 accumulators (conv + bias, no
 * activation, no fp16 rounding) written to out_f32 [n, oh, ow, cout].  Used by the engine's G1 mode (SURVEY 8d gate G1:
 * fp32 inter-layer storage, operands split into fp16 hi + lo parts, three launches per conv).  desc->relu / tail_* ignored
 * (tail_cout must be 0). */
LFD_API int lfd_conv2d_nhwc_f16_acc32(const lfd_conv_desc_t* desc, const void* in, float* out_f32, const void* w_packed,
                                      const float* bias, const void* zeros, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Large-map conv of the 256-channel FPN necks and head towers (csrc/conv256.hip): NHWC fp16, stride 1, pad ks/2, 256 input
 * channels, cout a multiple of 32 up to 256; fp32 accumulation on MFMA, one fixed summation order (no atomics, no workspace).
 * Replaces the nn.Conv2d units of the FPN output convs (lfd/model/neck/fpn.py:57-82), of the FCOSHead towers and output
 * convs (lfd/model/head/fcos_head.py:60-110,129-154) and of LFDHead's towers and output convs (lfd_head.py:97-117,164-185)
 * at num_output_channels / num_head_channels = 256; executed by cuDNN in the reference.
 *   out_f32 = 0: out [n,h,w,cout] fp16 = relu?( conv(in, w) + bias ), ks = 3.
 *   out_f32 = 1: out [n,h,w,cout] fp32 = relu?( conv(in, w) + bias ), the accumulators un-rounded (the heads' logits),
 *                ks = 3 or 1.
 * w_packed: lfd_pack_conv_weight_f16 order for (cin 256, cout, ks).  in / out / w_packed / bias 16-byte aligned.  h * w * 256
 * must stay below 2^31 (LFD_ERR_UNSUPPORTED otherwise); n * h * w * 256 may pass it.  lfd_conv256_nhwc_f16_supported answers
 * for a (cin, cout, ks, out_f32) key without launching. */
LFD_API int lfd_conv256_nhwc_f16_supported(int32_t cin, int32_t cout, int32_t ks, int32_t out_f32);
LFD_API int lfd_conv256_nhwc_f16(const void* in, void* out, const void* w_packed, const float* bias, int32_t n, int32_t h,
                                 int32_t w, int32_t cout, int32_t ks, int32_t relu, int32_t out_f32, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * INT8 deployment mode (csrc/conv_i8.hip; lfd_amd/deployment.py, lfd_amd/engine_i8.py): the convs of the residual
 * stages on v_mfma_i32_32x32x32_i8 with exact i32 accumulation and a requantising epilogue, and the quantise step behind the
 * fp16 stem.  Replaces what the reference obtains from TensorRT's INT8 builder and its INT8Calibrator
 * (lfd/deployment/tensorrt/build_engine.py:22-126); the calibration contract is this project's own (symmetric, per-output-
 * channel weight scales, one scale per activation tensor, range [-127, 127]).
 *
 * lfd_conv2d_nhwc_i8: desc = (n, h, w, cin, cout, ks, stride, relu) of an lfd_conv_desc_t (tail_cout must be 0); ks 1 | 3,
 * stride 1 | 2, pad ks / 2, cin and cout in {64, 128} (anything else: LFD_ERR_UNSUPPORTED, nothing written;
 * lfd_conv2d_nhwc_i8_supported answers for a key without launching).  in [n,h,w,cin] int8; w_packed: the fragment order of
 * lfd_amd.ops.pack_conv_weight_i8, cout * ks * ks * cin bytes; mult / biasq [cout] fp32; res [n,oh,ow,cout] int8 or NULL.
 * With acc the exact i32 sum:
 *   v = fmaf((float)acc, mult[co], biasq[co]);  res: v = fmaf((float)res, res_mult, v);  desc->relu: v = max(v, 0)
 *   out_i8  [n,oh,ow,cout] int8 = clamp(rint(v), -127, 127), round half even
 *   out_f16 [n,oh,ow,cout] fp16 = half(v * out_scale), the un-requantised value (a pyramid tap for the fp16 head), this v
 *           evaluated in float64 and rounded once (within one fp16 ulp of the exact value even where the residual add
 *           cancels); NULL: not written (out_scale ignored).
 * Every pointer 16-byte aligned; out_i8 must not alias in or res.  h * w * 128 must stay below 2^31.
 *
 * lfd_quantize_nhwc_f16_i8: out[i] = clamp(rint((float)in[i] * inv_scale), -127, 127) for i < count (any count >= 1); in fp16,
 * out int8, both 16-byte aligned.
 * lfd_quantize_pad_nhwc_f16_i8: the same step into wider pixels: out [pixels][cout] = the quantised in [pixels][cin] in channels
 * below cin and 0 above (a 32-channel stem in front of stages that run zero-padded to 64); cin, cout multiples of 16,
 * cin <= cout <= 128. */
LFD_API int lfd_conv2d_nhwc_i8_supported(int32_t cin, int32_t cout, int32_t ks, int32_t stride);
LFD_API int lfd_conv2d_nhwc_i8(const lfd_conv_desc_t* desc, const void* in, const void* w_packed, const float* mult,
                               const float* biasq, const void* res, float res_mult, void* out_i8, void* out_f16,
                               float out_scale, lfd_stream_t stream);
LFD_API int lfd_quantize_nhwc_f16_i8(const void* in, void* out, int64_t count, float inv_scale, lfd_stream_t stream);
LFD_API int lfd_quantize_pad_nhwc_f16_i8(const void* in, void* out, int64_t pixels, int32_t cin, int32_t cout, float inv_scale,
                                         lfd_stream_t stream);

/* Fused int8 launches (csrc/block_i8.hip and, the stride-2 pair, csrc/conv_i8.hip; the fused=True route of
 * lfd_amd/engine_i8.py).  Both equal the lfd_conv2d_nhwc_i8 launches they replace in every bit: the i32 sums are exact and the
 * epilogues are the expressions above (one definition, csrc/i8_impl.h).
 *
 * lfd_block_i8_fused: a whole residual block, y = ReLU(conv2(ReLU(conv1(x))) + x), both convs 3x3, stride 1, pad 1, 64 -> 64
 * channels.  in [n,h,w,64] int8; w1_packed / mult1 / biasq1 and w2_packed / mult2 / biasq2: the operands of the two
 * lfd_conv2d_nhwc_i8 calls (the same fragment order: nothing is repacked); res_mult: conv2's, for the identity x.
 *   mid     = clamp(rint(max(fmaf((float)acc1, mult1[c], biasq1[c]), 0)), -127, 127), int8, never written to memory; mid pixels
 *             outside the image are conv2's zero padding (0, not conv1 evaluated there)
 *   v       = max(fmaf((float)x, res_mult, fmaf((float)acc2, mult2[c], biasq2[c])), 0)
 *   out_i8  [n,h,w,64] int8 = clamp(rint(v), -127, 127)
 *   out_f16 [n,h,w,64] fp16 = half(v * out_scale), this v evaluated in float64 as lfd_conv2d_nhwc_i8 does; NULL: not written.
 * LFD_ERR_INVALID_ARGUMENT: a NULL pointer (but out_f16), a pointer that is not 16-byte aligned, n / h / w < 1, out_i8 == in.
 * LFD_ERR_UNSUPPORTED: h * w * 128 >= 2^31.  A refused call launches and writes nothing.
 *
 * lfd_conv2d_downsample_nhwc_i8: the two stride-2 convs that open a stage-entry block, from one staged input tile:
 *   out_i8    [n,oh,ow,cout] = the 3x3 stride-2 pad-1 conv (w_packed, mult, biasq) with ReLU
 *   ds_out_i8 [n,oh,ow,cout] = the 1x1 stride-2 identity branch (ds_w_packed, ds_mult, ds_biasq) without ReLU
 * oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1; each output follows the epilogue of lfd_conv2d_nhwc_i8 without residual, with
 * its own constants and therefore its own output scale; no fp16 tap.  (cin, cout) in {(64, 64), (64, 128), (128, 128)}, anything
 * else LFD_ERR_UNSUPPORTED (lfd_conv2d_downsample_nhwc_i8_supported answers without launching).  Pointers 16-byte aligned, the
 * three tensors distinct, h * w * 128 < 2^31; status codes as above. */
LFD_API int lfd_block_i8_fused(int32_t n, int32_t h, int32_t w, const void* in, const void* w1_packed, const float* mult1,
                               const float* biasq1, const void* w2_packed, const float* mult2, const float* biasq2,
                               float res_mult, void* out_i8, void* out_f16, float out_scale, lfd_stream_t stream);
/* lfd_block128_i8_fused (csrc/block128_i8.hip; the block128 option of lfd_amd/engine_i8.py): the 128-channel sibling of
 * lfd_block_i8_fused with the same signature and the same contract, 128 for 64: in, out_i8 and out_f16 are [n,h,w,128], the
 * operands are those of the two 128 -> 128 lfd_conv2d_nhwc_i8 calls in the same fragment order, mid is int8, never written to
 * memory and 0 outside the image, out_i8 = q(v), out_f16 = half(v * out_scale) with v in float64 (NULL: not written).  The
 * requantisation is lfd_conv2d_nhwc_i8's own compare / select form, so the launch equals the two it replaces in every bit,
 * NaN constants included.  Status codes as for lfd_block_i8_fused; a refused call launches and writes nothing. */
LFD_API int lfd_block128_i8_fused(int32_t n, int32_t h, int32_t w, const void* in, const void* w1_packed, const float* mult1,
                                  const float* biasq1, const void* w2_packed, const float* mult2, const float* biasq2,
                                  float res_mult, void* out_i8, void* out_f16, float out_scale, lfd_stream_t stream);
LFD_API int lfd_conv2d_downsample_nhwc_i8_supported(int32_t cin, int32_t cout);
LFD_API int lfd_conv2d_downsample_nhwc_i8(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, const void* in,
                                          const void* w_packed, const float* mult, const float* biasq, const void* ds_w_packed,
                                          const float* ds_mult, const float* ds_biasq, void* out_i8, void* ds_out_i8,
                                          lfd_stream_t stream);

/* One-launch 64-channel stage-entry block (csrc/entry_i8.hip; the fused='full' route of lfd_amd/engine_i8.py): the 3x3 stride-2
 * conv1 (ReLU), the 1x1 stride-2 identity branch (no ReLU) and the 3x3 stride-1 conv2 that adds it (ReLU), all 64 -> 64 (padded)
 * channels, with the operands of the lfd_conv2d_downsample_nhwc_i8 + lfd_conv2d_nhwc_i8 launches it replaces (the same fragment
 * order: nothing is repacked) and equal to them in every bit for finite inputs (finite in and in_inv_scale, finite epilogue
 * constants): a NaN, which those launches turn into 0, becomes -127 or 127 here; +/-inf saturates alike in both.
 * oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1.
 *   in_format 0: in int8 [n,h,w,64], xq = in; in_channels must be 64, in_inv_scale is ignored
 *   in_format 1: in fp16 [n,h,w,in_channels], in_channels in {32, 48, 64}; xq = clamp(rint((float)x * in_inv_scale), -127, 127)
 *                in channels < in_channels and 0 above: lfd_quantize_nhwc_f16_i8 / lfd_quantize_pad_nhwc_f16_i8 on the way in
 *   y1  = q(max(fmaf((float)acc1, mult1[c], biasq1[c]), 0)), 3x3 stride 2 pad 1 over xq, int8, never written to memory
 *   id  = q(fmaf((float)accd, ds_mult[c], ds_biasq[c])), 1x1 stride 2, int8, never written to memory
 *   v   = max(fmaf((float)id, res_mult, fmaf((float)acc2, mult2[c], biasq2[c])), 0), acc2 the 3x3 stride-1 pad-1 sum over y1 with
 *         0 outside the oh x ow map (conv2's padding, not conv1 evaluated there)
 *   out_i8 [n,oh,ow,64] = q(v), q(.) = clamp(rint(.), -127, 127).  There is no fp16 tap output.
 * LFD_ERR_INVALID_ARGUMENT: a NULL pointer, a pointer that is not 16-byte aligned, n / h / w < 1, out_i8 == in.
 * LFD_ERR_UNSUPPORTED: another format or channel count (lfd_entry_i8_fused_supported answers without launching), or
 * h * w * 128 >= 2^31.  A refused call launches and writes nothing. */
LFD_API int lfd_entry_i8_fused(int32_t n, int32_t h, int32_t w, int32_t in_format, int32_t in_channels, const void* in,
                               float in_inv_scale, const void* w1_packed, const float* mult1, const float* biasq1,
                               const void* ds_w_packed, const float* ds_mult, const float* ds_biasq, const void* w2_packed,
                               const float* mult2, const float* biasq2, float res_mult, void* out_i8, lfd_stream_t stream);
LFD_API int lfd_entry_i8_fused_supported(int32_t in_format, int32_t in_channels);

/* ------------------------------------------------------------------------------------------
 * INT8 calibration histogram (csrc/calib_hist.hip; lfd_amd/calibration.py): the counts from which the percentile,
 * entropy and MSE thresholds are computed on the host.  Stands where the reference hands its calibration batches to
 * tensorrt.IInt8EntropyCalibrator2 (lfd/deployment/tensorrt/build_engine.py:22).
 *
 * lfd_abs_histogram_f16: x [rows, c] fp16; hist[bits(x[r][ch]) & 0x7fff] += 1 for every r < rows and ch < c_real.  The 32768
 * bins are the fp16 magnitudes themselves (+0 and -0 share bin 0; the Inf and NaN patterns, bins >= 0x7c00, are counted in
 * their own bins: judging them is the caller's business).  Channels c_real .. c - 1 (the plan's zero padding) are not counted,
 * whatever they hold.  hist [32768] uint64 on the device is added to, never cleared: calls accumulate.  Integer sums do not
 * depend on the order, so equal inputs give equal bits.
 * c % 8 == 0, 1 <= c_real <= c, rows >= 0, x 16-byte aligned, hist 8-byte aligned (LFD_ERR_INVALID_ARGUMENT otherwise);
 * rows == 0 returns LFD_OK and launches nothing.  A workgroup counts in 32-bit bins and flushes them once, at its end: a map
 * of more than 2^39 elements (rows * c), whose share per workgroup could wrap a bin, is refused with LFD_ERR_UNSUPPORTED
 * (nothing written) rather than flushed early -- split such a map by rows.
 * Geometry (restated by the tests): at most LFD_CALIB_HIST_MAX_WORKGROUPS workgroups, each walking chunks of
 * LFD_CALIB_HIST_CHUNK_VECS 16-byte vectors (8 elements each) with the grid as stride. */
#define LFD_CALIB_HIST_MAX_WORKGROUPS 256
#define LFD_CALIB_HIST_CHUNK_VECS 4096
LFD_API int lfd_abs_histogram_f16(const void* x, int64_t rows, int32_t c, int32_t c_real, uint64_t* hist, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 'fp32_storage' precision mode of the eval forward (LFD.precision = 'fp32_storage'): a shipped mode of the product for
 * callers that need the reference's fp32 outputs to <= 1e-4 on the raw logits (north_star: "cls/bbox tensors within
 * 1e-3"); replaces the same reference code as the fp16 entry points above -- nn.Conv2d + eval BatchNorm2d (+ residual)
 * + ReLU of lfd_resnet.py:354-501 / simple_neck.py:67-74, the head convs, GroupNorm + ReLU and Scale of
 * lfd_head.py:97-117,164-185.  Activations are fp32 NHWC; ONE launch per conv: operands are split exactly into fp16
 * hi + 2^-11 lo parts inside the kernel (activations by the tile loader, weights once per plan), three MFMAs per k-step,
 * fp32 accumulation, epilogue out = relu?( scale * (conv + bias (+ residual)) ) in fp32.
 *   in_format < 0: `in` is fp32 NHWC [n,h,w,cin], cin a multiple of 32; ks 1|3, stride 1|2, pad ks/2.
 *   in_format 0|1|2 (NCHW fp32 / NHWC fp16 / NHWC uint8 + simple_normalize): the first stem conv, 3x3 stride 2 on the
 *     3-channel frame (cin = 3); the 27 taps are one 32-wide k chunk gathered from the frame.  cin = 1: a one-channel frame
 *     (NCHW [n,1,h,w] and NHWC [n,h,w,1] are the same bytes), its 9 taps k = dy*3 + dx in the same 32-wide chunk.
 *   w_packed: lfd_p32_conv_packed_weight_halfs() fp16 values, [cout/32 slabs][cin/32 chunks][ks*ks taps][2 k-steps]
 *     [hi | 2^11 lo][64 lanes][8]; lane = 32 * khalf + cout_local, element j = channel 32 chunk + 16 kstep + 8 khalf + j
 *     (first conv: k = (dy*3 + dx)*cin + c, zero from 9*cin on); bias [32 * slabs] fp32 (zero padded).
 *   out: channel c of pixel (oy, ox) of image i at out[i * out_image_stride + (oy*OW + ox) * out_pixel_stride + c]
 *     (0 = dense: out_pixel_stride = cout, out_image_stride = OH*OW*cout) -- the head's output convs write straight into
 *     the level-concatenated [N,P,C'] / [N,P,4] tensors (lfd.py:526-542); residual: dense fp32 [n,OH,OW,cout] or NULL;
 *     scale: device pointer to ONE float (lfd_head.py Scale, applied after the bias) or NULL. */
typedef struct lfd_p32_conv_desc {
  int32_t n, h, w, cin, cout, ks, stride, relu;
  int32_t in_format;
  int32_t out_pixel_stride;
  int64_t out_image_stride;
} lfd_p32_conv_desc_t;
LFD_API size_t lfd_p32_conv_packed_weight_halfs(int32_t cin, int32_t cout, int32_t ks);
LFD_API int lfd_p32_conv2d_nhwc_f32(const lfd_p32_conv_desc_t* desc, const void* in, float* out, const void* w_packed,
                                    const float* bias, const float* residual, const float* scale, lfd_stream_t stream);
/* the same conv chained with a 1x1 conv 64 -> 64 in ONE launch: out = relu?( conv1x1( relu?(conv(in) + bias) ) + tail_bias )
 * -- the stem pairs conv3x3 s2 + BN + ReLU -> conv1x1 + BN + ReLU (lfd_resnet.py:356-413); the 64-channel fp32 intermediate
 * stays in LDS.  desc->cout must be 64, the conv 3x3 stride 2 (in_format < 0) or the first stem conv (in_format 0|1|2);
 * tail_w_packed = lfd_p32_conv_packed_weight_halfs(64, 64, 1) halfs in the same layout. */
LFD_API int lfd_p32_conv2d_tail_nhwc_f32(const lfd_p32_conv_desc_t* desc, const void* in, float* out, const void* w_packed,
                                         const float* bias, const void* tail_w_packed, const float* tail_bias, int32_t tail_relu,
                                         lfd_stream_t stream);
/* x [n, hw, c] fp32 <- relu?( GroupNorm(groups)(x) * gamma + beta ) in place (nn.GroupNorm semantics: biased variance
 * over hw x c/groups elements per image and group; statistics summed in fp64 in a fixed order); c % 4 == 0,
 * 256 % (c/4) == 0, (c/groups) % 4 == 0, groups <= 64. */
LFD_API size_t lfd_p32_groupnorm_workspace_bytes(int32_t n, int32_t groups);
LFD_API int lfd_p32_groupnorm_relu_f32(float* x, int32_t n, int64_t hw, int32_t c, int32_t groups, const float* gamma,
                                       const float* beta, float eps, int32_t relu, void* workspace, size_t workspace_bytes,
                                       lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same mode for the pyramid necks and FCOSHead (FCOS / LFDv2 / LFD over FPN, SimpleFPN, LFDHeadV1:
 * lfd_amd/engine_sibling_p32.py; csrc/precise.hip, csrc/precise_pyramid.hip).  Dense fp32 NHWC tensors, 16-byte aligned,
 * channels a multiple of 4; nothing is launched when a status code is returned.
 *   lfd_p32_conv2d_merge_nhwc_f32      replaces a lateral 1x1 conv (+ folded BatchNorm, + ReLU) AND the top-down merge that
 *                                      follows it, `lateral[i-1] += nn.Upsample(size, mode='nearest')(lateral[i])`
 *                                      (lfd/model/neck/fpn.py:127-152, simple_fpn.py:141-172), in one launch:
 *                                      out = relu?(conv + bias) + nearest(up [n, up_h, up_w, cout]) -- the ReLU
 *                                      (relu_on_lateral) before the add, as the reference orders them.  desc: in_format < 0,
 *                                      ks 1, stride 1, dense output, cout % 4 == 0; up_h <= h, up_w <= w; `up` is the coarser
 *                                      level AFTER its own merge (walk the laterals from the coarsest down).  The same bits as
 *                                      lfd_p32_conv2d_nhwc_f32 followed by lfd_p32_upsample_nearest_add_f32.
 *   lfd_p32_upsample_nearest_add_f32   the merge step alone (same reference lines): dst[n,H,W,c] += nearest(src[n,h,w,c]),
 *                                      source index min(floorf(dst_index * float(in)/out), in-1) as ATen computes it (the rule
 *                                      of lfd_upsample_nearest_add_nhwc_f16); h <= H, w <= W, equal sizes are a plain add.
 *   lfd_p32_relu_f32                   nn.ReLU(inplace=True) in front of an extra level (fpn.py:127-152 / simple_fpn.py:141-172
 *                                      run `fpn_out{i}` = Sequential(ReLU(inplace=True), ...) on the previous output, which it
 *                                      rewrites as well).
 *   lfd_p32_maxpool3x3s2_f32           extra_type='pooling': nn.MaxPool2d(3, 2, 1) (same lines) -> [n, (h+1)/2, (w+1)/2, c];
 *                                      F.max_pool2d semantics at the border (the padding never wins).
 *   lfd_p32_exp_rows_f32               replaces the `.float().exp()` of `scales[i](regression(x)).float().exp()`
 *                                      (lfd/model/head/fcos_head.py:129-154); conv, bias and Scale are the epilogue of
 *                                      lfd_p32_conv2d_nhwc_f32 writing rows row0 .. row0+rows of the level-concatenated
 *                                      out [n, P, c] (image_stride = P * c floats); this entry applies expf (not the fast
 *                                      intrinsic) to those rows of every image in place and touches nothing else. */
LFD_API int lfd_p32_conv2d_merge_nhwc_f32(const lfd_p32_conv_desc_t* desc, const void* in, float* out, const void* w_packed,
                                          const float* bias, const float* up, int32_t up_h, int32_t up_w, lfd_stream_t stream);
LFD_API int lfd_p32_upsample_nearest_add_f32(float* dst, const float* src, int32_t n, int32_t H, int32_t W, int32_t h,
                                             int32_t w, int32_t c, lfd_stream_t stream);
LFD_API int lfd_p32_relu_f32(float* x, int64_t count, lfd_stream_t stream);
LFD_API int lfd_p32_maxpool3x3s2_f32(const float* in, float* out, int32_t n, int32_t h, int32_t w, int32_t c,
                                     lfd_stream_t stream);
LFD_API int lfd_p32_exp_rows_f32(float* out, int32_t n, int64_t image_stride, int64_t row0, int64_t rows, int32_t c,
                                 lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same precision mode on "hi/lo planes" (csrc/planes.hip, csrc/planes_impl.h; lfd_amd/engine_p2.py) -- the fast form of
 * the mode inside north_star's 1e-3 (lfd/model/lfd.py:511-542 to <= 1e-4 on the raw logits).
 * A plane tensor stores an fp32-valued NHWC activation x as two contiguous NHWC fp16 tensors: hi = fp16(x) at the base pointer,
 * lo = fp16(2^11 (x - hi)) `*_plane_halfs` halfs behind it (x = hi + 2^-11 lo to ~22 bits; the bytes of fp32).  Both planes are
 * 16-byte aligned, plane strides multiples of 8 halfs.  Convolutions are weights-stationary LDS-DMA kernels issuing three
 * fp16 MFMAs per k-step (w_hi x_hi | w_hi x_lo + w_lo x_hi), fp32 accumulation, fp32 epilogue, split on the way out.
 * Packed weights of every entry point: [2 = hi | 2^11 lo][fragments of lfd_conv_packed_weight_halfs order], rows zero-padded
 * to a multiple of 32 (engine_p2.pack_planes_weight); biases fp32 padded likewise.
 * RANGE: a plane pair has the PRECISION of ~22 bits but the RANGE of fp16 -- |x| <= 65504; the split does not saturate, a larger
 * value stores hi = +-inf and reads back as NaN (the fp32-tensor form of the mode, lfd_p32_*, has fp32's range and is what to use
 * for a network whose activations exceed it; BatchNorm / GroupNorm-normalised LFD activations stay below ~1e2).  The fixed-point
 * GroupNorm sums (2^-24 units in int64) hold a group's sum of squares up to ~5.5e11.  Where the text below says "statistics in
 * fp64": a thread adds the <= 64 values it copies out of ONE tile in fp32, tiles are combined in fp64, workgroups in fixed point.
 *
 * lfd_pl_stem_pair: frame (in_format as lfd_stem_conv_f16) -> conv3x3 s2 (3 -> C) + BN + ReLU -> conv1x1 (C -> C) + BN + ReLU
 *   -> planes [n, (h+1)/2, (w+1)/2, C], C = 32 | 64 (lfd_resnet.py:356-374, :376-395).  w1: [2][C/32][2][64][8] in
 *   engine.pack_stem_weight order per plane.  uint8 / fp32 frames keep their low parts (simple_normalize in fp32).
 * lfd_pl_stem2x: the whole 'faster' stem (lfd_resnet.py:376-413), frame -> planes [n, ceil(ceil(h/2)/2), ceil(ceil(w/2)/2), 64]
 *   in one launch: the second pair's persistent workgroups compute their input tile from the frame in LDS, the first pair's
 *   output (the largest tensor of the network) never exists in HBM.  w1: conv0 AND its bias, [2][2 slabs][2 k-steps][64 lanes][8]
 *   in the k-slot order of the fused gather (engine_p2.pack_planes_stem2x_weight: per frame row the 10 halfs [pixel left of the
 *   patch, e0..e8], e = 3 dx + c, as aligned dwords; the bias on the slot of a constant one); w2: the first 1x1 with K in the
 *   order the conv0 accumulators hold the channels (engine_p2.pack_planes_stem2x_tail_weight), b2 its bias [64]; w3 / w4:
 *   lfd_pl_conv2d order (3x3 s2 64 -> 64, 1x1 64 -> 64), b3 / b4 [128] zero padded.
 *   fp16 NHWC frames with w % 8 == 0, uint8 NHWC frames with w % 16 == 0 and fp32 NCHW frames with w % 4 == 0, on a 16-byte aligned
 *   base, run k_pl_stem2xs (round 6: a row stream down strips of 16 output columns, producer waves and consumer waves, the frame
 *   patch by 16-byte LDS-DMA; uint8 values through a 256-entry table of split simple_normalize values, fp32 values split at the
 *   gather; planes_stem2xs.hip; the tuning knob PL_STEM set to 0 selects the tile kernel for them too); other widths / alignments run
 *   the tile kernel k_pl_stem2x with loads.  Both kernels take the same packed filters; their results differ by the order of fp32 sums (<= 2e-6 at 8 x 1080p).
 * lfd_pl_conv2d: planes [n,h,w,cin] -> conv ks x ks / stride (+ bias, ReLU) with ONE of
 *     tail_cout > 0   : a chained 1x1 cout -> cout (+ tail_bias, tail_relu) in the same launch (the intermediate stays in LDS):
 *                       the second stem pair (3x3 s2 -> 1x1, lfd_resnet.py:396-413), the neck conv -> first tower conv;
 *     ds_w_packed     : second output ds_out = conv1x1 stride 2 (in) + ds_bias, no ReLU -- the identity branch of a stage's
 *                       first block (lfd_resnet.py:458-468) from the centre tap of a 3x3 stride-2 conv;
 *     residual        : y += residual (planes, same shape as out) before the ReLU (lfd_resnet.py:151-152);
 *   out_mode 0: planes out.  1: planes out + GroupNorm sums: gn_sums[((replica * n + image) * cout/8 + group) * 2 + {0,1}] +=
 *   {sum, sum of squares} of the stored values of that 8-channel group as 64-bit two's-complement fixed point (2^-24
 *   units), replica = workgroup % LFD_PL_GN_REPLICAS (LFD_PL_GN_REPLICAS * n * cout/8 * 2 words; consumers add the replicas)
 *   -- order-independent integer atomics, so the statistics are bit-reproducible; the caller zeroes gn_sums per forward.  2: fp32
 *   outputs without planes: channel c < f_c0 -> f_out0[image * f_image_stride0 + pixel * f_c0 + c], f_c0 <= c < f_c0 + f_c1
 *   -> f_out1[image * f_image_stride1 + pixel * f_c1 + c - f_c0] * (*scale1) (lfd_head.py:176-183: cls / reg convs + Scale
 *   straight into the level-concatenated [N,P,C'] / [N,P,4] tensors, lfd.py:526-542).
 *   gn_in_sums != NULL (1x1 convs on 128 channels): the input planes are the PRE-normalisation output of the conv that
 *   accumulated gn_in_sums; the landed tile is normalised (GroupNorm(16, 128), gn_in_gamma / gn_in_beta / desc->gn_in_eps,
 *   mean / rstd in fp64 from the sums) + ReLU'd in LDS before the contraction -- the tower's conv -> GroupNorm -> ReLU
 *   (lfd_head.py:97-117) without a pass over the tensor.
 *   Supported shapes: the layers of every named configuration (see the dispatch in csrc/planes.hip); LFD_ERR_UNSUPPORTED
 *   otherwise -- the host falls back to lfd_p32_*.  zeros: the 4 KB line of lfd_conv2d_nhwc_f16.
 * lfd_pl_conv2d_levels: the same 1x1 conv (desc: n, cin, cout, relu, tail_cout / tail_relu, out_mode, f_c0 / f_c1,
 *   f_image_stride0 / 1, gn_in_eps; ks = stride = 1; desc->h / w / *_plane_halfs unused) over num_levels <= LFD_MAX_LEVELS
 *   feature maps in ONE launch -- simple_neck.py:67-74 + lfd_head.py:164-185 apply the same conv stack to every pyramid
 *   level, each level with its own filters; levels[i] carries what lfd_pl_conv2d takes per call.  Results are identical to
 *   num_levels lfd_pl_conv2d calls: same arithmetic per tile; the GroupNorm sums are order-independent integers (which
 *   REPLICA a workgroup adds to depends on the grid -- the statistic is the sum over the replicas).
 * lfd_pl_groupnorm_relu: x (planes [n, hw, c]) <- relu?(GroupNorm(c/8 groups)(x) * gamma + beta) in place, mean / rstd in
 *   fp64 from gn_sums (lfd_head.py:97-117 conv -> GroupNorm -> ReLU). */
#define LFD_PL_GN_REPLICAS 8   /* gn_sums holds this many replicas of [n][cout/8][2]: a producer spreads its atomics, consumers add */
typedef struct lfd_pl_conv_desc {
  int32_t n, h, w, cin, cout, ks, stride, relu;
  int32_t tail_cout, tail_relu;
  int32_t out_mode;
  int32_t f_c0, f_c1;
  float gn_in_eps;
  int64_t in_plane_halfs, out_plane_halfs, res_plane_halfs, ds_plane_halfs;
  int64_t f_image_stride0, f_image_stride1;
} lfd_pl_conv_desc_t;
LFD_API int lfd_pl_stem_pair(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels,
                             const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                             int64_t out_plane_halfs, lfd_stream_t stream);
LFD_API int lfd_pl_stem2x(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, const void* w1_packed,
                          const void* w2_packed, const float* b2, const void* w3_packed, const float* b3,
                          const void* w4_packed, const float* b4, void* out, int64_t out_plane_halfs, const void* zeros,
                          lfd_stream_t stream);
LFD_API int lfd_pl_conv2d(const lfd_pl_conv_desc_t* desc, const void* in, void* out, const void* w_packed, const float* bias,
                          const void* residual, const void* tail_w_packed, const float* tail_bias, const void* ds_w_packed,
                          const float* ds_bias, void* ds_out, void* gn_sums, float* f_out0, float* f_out1, const float* scale1,
                          const void* gn_in_sums, const float* gn_in_gamma, const float* gn_in_beta, const void* zeros,
                          lfd_stream_t stream);
/* lfd_pl_block64: one residual block of the planes mode (lfd_resnet.py:96-154 without a downsample branch) in ONE launch:
 *   m = planes(ReLU(conv3x3(in) + b1)),  out = planes(ReLU(conv3x3(m) + b2 + in)),  64 -> 64 -> 64 channels, stride 1, pad 1.
 *   in / out: planes [n,h,w,64] (hi plane, the lo plane in_plane_halfs / out_plane_halfs behind it), not overlapping;
 *   w1_packed / w2_packed: lfd_pl_conv2d order [2][2][36][64] x 8 halfs; b1 / b2: [>= 64] fp32; zeros: the 4 KB line of
 *   lfd_conv2d_nhwc_f16.  csrc/planes_block.hip (k_pl_blk64: a row stream down strips of 30 output columns, the
 *   intermediate m in LDS only).  Bit-identical to two lfd_pl_conv2d launches (conv1, then conv2 with residual = in) under
 *   the default tuning of
 *   the 3x3 plane convs (k_pl_c3p).  Any n, h, w >= 1; LFD_ERR_INVALID_ARGUMENT for null / misaligned / overlapping
 *   buffers or short planes. */
LFD_API int lfd_pl_block64(int32_t n, int32_t h, int32_t w, const void* in, int64_t in_plane_halfs, void* out,
                           int64_t out_plane_halfs, const void* w1_packed, const float* b1, const void* w2_packed,
                           const float* b2, const void* zeros, lfd_stream_t stream);
typedef struct lfd_pl_level {
  const void* in;                 /* planes [n, h, w, cin] */
  void* out;                      /* planes [n, h, w, cout] (out_mode 0 | 1) */
  const void* w_packed;
  const float* bias;
  const void* tail_w_packed;      /* desc->tail_cout > 0 */
  const float* tail_bias;
  void* gn_sums;                  /* out_mode 1 */
  const void* gn_in_sums;         /* all levels or none */
  const float* gn_in_gamma;
  const float* gn_in_beta;
  float* f_out0;                  /* out_mode 2 */
  float* f_out1;
  const float* scale1;
  int32_t h, w;
  int64_t in_plane_halfs, out_plane_halfs;
} lfd_pl_level_t;
LFD_API int lfd_pl_conv2d_levels(const lfd_pl_conv_desc_t* desc, const lfd_pl_level_t* levels, int32_t num_levels,
                                 const void* zeros, lfd_stream_t stream);
LFD_API int lfd_pl_groupnorm_relu(void* x, int64_t plane_halfs, int32_t n, int64_t hw, int32_t c, const void* gn_sums,
                                  const float* gamma, const float* beta, float eps, int32_t relu, lfd_stream_t stream);

/* lfd_pl_head_levels (round 6, csrc/planes_head.hip): the neck + head 1x1 convs of the planes mode (simple_neck.py:67-74,
 * lfd_head.py:88-139,164-185, lfd.py:526-542) over FLAT pixel lists -- a pyramid level of an image is `pixels` = h * w pixels,
 * tiles of 64, all levels of a launch in one persistent grid, every level with its own filters.  The pre-GroupNorm outputs of
 * the tower convs are private to these launches and stored as plain fp32 [n][pixels][128] (the bytes of a plane pair).
 *   mode 0: in = planes [n][pixels][cin] (cin 64 | 128, the backbone tap) -> conv w0 (cin -> 128) + b0 (+ ReLU if relu0) ->
 *           conv w1 (128 -> 128) + b1 -> out fp32, gn_sums += {sum, sum of squares} of out per (image, 8-channel group)
 *           in the fixed-point replica layout of lfd_pl_conv2d (caller zeroes gn_sums per forward)
 *   mode 1: in = fp32 [n][pixels][128] + its producer's gn_in_sums / gamma / beta (GroupNorm(16, 128), eps) -> ReLU ->
 *           conv w0 (128 -> 128) + b0 -> out fp32, gn_sums as above
 *   mode 2: in as mode 1 -> conv w0 (128 -> f_c0 + f_c1 <= 64 channels, packed to 32 | 64 rows) + b0 -> fp32 outputs as
 *           lfd_pl_conv2d out_mode 2 (f_out0 / f_out1 at the level's point offset, image strides f_image_stride0 / 1, scale1)
 *   mode 3: in = planes [n][pixels][128] (the stored output of a neck conv: heads with separate cls / reg towers) -> conv w0
 *           (128 -> 128) + b0 -> out fp32, gn_sums as mode 0
 * Packed weights: engine_p2.pack_planes_weight order ([2 = hi | 2^11 lo][cout / 32][cin / 16][64 lanes] x 8 halfs). */
typedef struct lfd_pl_head_desc {
  int32_t mode, n, cin, relu0;
  int32_t f_c0, f_c1;
  float gn_in_eps;
  int32_t pad_;
  int64_t f_image_stride0, f_image_stride1;
} lfd_pl_head_desc_t;
typedef struct lfd_pl_head_level {
  const void* in;
  void* out;                      /* fp32 [n][pixels][128] (modes 0, 1) */
  const void* w0;
  const float* b0;
  const void* w1;                 /* mode 0 */
  const float* b1;
  void* gn_sums;                  /* modes 0, 1 */
  const void* gn_in_sums;         /* modes 1, 2 */
  const float* gn_in_gamma;
  const float* gn_in_beta;
  float* f_out0;                  /* mode 2 */
  float* f_out1;
  const float* scale1;
  int64_t in_plane_halfs;         /* mode 0 */
  int32_t pixels, pad_;
} lfd_pl_head_level_t;
LFD_API int lfd_pl_head_levels(const lfd_pl_head_desc_t* desc, const lfd_pl_head_level_t* levels, int32_t num_levels,
                               const void* zeros, lfd_stream_t stream);

/* First stem unit: conv3x3 s2 (3 -> C) + BN + ReLU chained with conv1x1 (C -> C) + BN + ReLU
 * (lfd_resnet.py:356-374 'fast' stem; first half of the 'faster' stem :376-395).
 * in_format: 0 = NCHW fp32 (the tensor LFD.forward receives, lfd.py:511), 1 = NHWC fp16,
 * 2 = NHWC uint8 with simple_normalize (x/255-0.5)/0.5 fused (augmentation_pipeline.py:31-36).
 * w2_packed == NULL: no chained 1x1.  out: NHWC fp16 [n, (h+1)/2, (w+1)/2, channels]. */
LFD_API int lfd_stem_conv_f16(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w,
                              int32_t channels, const void* w1_packed, const float* b1,
                              const void* w2_packed, const float* b2, void* out, lfd_stream_t stream);

/* The same unit writing the int8 map the INT8 mode's stages read (the stem_int8 option of lfd_amd/engine_i8.py): for
 * every output element, with y the fp16 value lfd_stem_conv_f16 stores (after bias and ReLU),
 *   out = clamp(rint((float)y * inv_scale), -127, 127), int8 NHWC [n, (h+1)/2, (w+1)/2, 64],
 * rint half to even, (float)y * inv_scale one fp32 multiply: lfd_quantize_nhwc_f16_i8's expression, evaluated on the fp16
 * value.  Equal in every bit to lfd_stem_conv_f16 followed by lfd_quantize_nhwc_f16_i8 for finite y and finite inv_scale; a
 * NaN becomes 0, as it does there.  The fp16 map is not written.
 * All three in_formats; channels == 64 and the chained 1x1 (w2_packed != NULL) only: everything else is LFD_ERR_UNSUPPORTED
 * (lfd_stem_conv_i8_supported(in_format, channels, has_tail) answers without launching).  out, w1_packed, b1, w2_packed, b2:
 * 16-byte aligned.  LFD_ERR_INVALID_ARGUMENT: a NULL in / w1_packed / b1 / out, w2_packed given without b2 or the reverse, a
 * misaligned pointer, n / h / w < 1 -- checked on the host before any launch.  A refused call launches and writes nothing. */
LFD_API int lfd_stem_conv_i8(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels,
                             const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, float inv_scale,
                             void* out, lfd_stream_t stream);
LFD_API int lfd_stem_conv_i8_supported(int32_t in_format, int32_t channels, int32_t has_tail);

/* First layer of the torchvision-style ResNet: conv7x7 stride 2 pad 3 (3 -> 64) + BatchNorm (folded on the host) + ReLU on a
 * frame (resnet.py:366-370, :470-473; csrc/stem7.hip).  in_format as lfd_stem_conv_f16 (uint8: simple_normalize on the load).
 * w_packed: [2 = co / 32][10 k-steps][64 lanes][8] fp16, lane (hk, co % 32) slot j of k-step s = tap slot k = 16 s + 8 hk + j:
 *   s < 7:  filter row ky = s, e = 8 hk + j                                   (e = 3 kx + c)
 *   s >= 7: i = 8 (2 (s - 7) + hk) + j < 35: ky = i / 5, e = 16 + i % 5;  i >= 35: zero
 * (engine_resnet.pack_stem7_weight); lfd_stem7_packed_weight_halfs() = 64 * 160 is its size.  bias fp32 [64].
 * out: NHWC fp16 [n, (h+1)/2, (w+1)/2, 64].  The max-pool that follows is lfd_maxpool3x3s2_nhwc_f16.
 * w_packed, bias, out: 16-byte aligned.  LFD_ERR_INVALID_ARGUMENT: a null pointer, n / h / w < 1, an in_format other than
 * 0..2, misalignment -- checked on the host before any launch. */
LFD_API int lfd_stem7_conv_f16(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, const void* w_packed,
                               const float* bias, void* out, lfd_stream_t stream);
LFD_API size_t lfd_stem7_packed_weight_halfs(void);

/* First stem unit of a one-channel (grayscale, input_channels = 1) model: conv3x3 s2 (1 -> C) + BN + ReLU, chained with
 * conv1x1 (C -> C) + BN + ReLU when w2_packed != NULL (lfd_resnet.py:356-374 'fast' stem; first half of the 'faster' stem
 * :376-395; csrc/stem_gray.hip).  The frame is one [n, h, w] plane -- NCHW [n,1,h,w] and NHWC [n,h,w,1] are the same bytes:
 * in_format 0 = fp32, 1 = fp16, 2 = uint8 with simple_normalize (x/255-0.5)/0.5 in fp32 on the load.  channels 32 | 64.
 * w1_packed: [C/32][64 lanes][8] fp16, lane (h, co) slot j = tap k = 8 h + j (k = 3 ky + kx < 9, other slots zero;
 * engine.pack_stem_gray_weight); w2_packed: lfd_conv2d 1x1 order (ops.pack_conv_weight), b1 / b2 fp32 [C].
 * lfd_stem_gray_f16: out NHWC fp16 [n, (h+1)/2, (w+1)/2, C], the numerics of lfd_stem_conv_f16.
 * lfd_pl_stem_gray_pair: out hi/lo planes (the plane layout of lfd_pl_stem_pair, out_plane_halfs a multiple of 8 and at least
 *   one plane's size); w1 / w2 [2 = hi | 2^11 lo][...] as above per plane; uint8 / fp32 frames keep their low parts.
 * out, b1, b2: 16-byte aligned.  LFD_ERR_INVALID_ARGUMENT: a null pointer (b2 must be given iff w2_packed is), sizes < 1, an
 * in_format other than 0..2, misalignment, a bad plane stride; LFD_ERR_UNSUPPORTED: channels not 32 | 64. */
LFD_API int lfd_stem_gray_f16(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels,
                              const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                              lfd_stream_t stream);
LFD_API int lfd_pl_stem_gray_pair(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels,
                                  const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                                  int64_t out_plane_halfs, lfd_stream_t stream);

/* The whole 'faster' stem (lfd_resnet.py:376-413) in one kernel: conv3x3 s2 (3->C), conv1x1, conv3x3 s2
 * (C->C), conv1x1, each + BN + ReLU.  The stride-2 intermediate (the largest activation of the
 * network) is produced tile-by-tile into LDS and never written to HBM (csrc/stem_fused.hip).
 * out: NHWC fp16 [n, ceil(ceil(h/2)/2), ceil(ceil(w/2)/2), channels]; channels in {32, 64}. */
LFD_API int lfd_stem_faster_fused_f16(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w,
                                      int32_t channels, const void* w1_packed, const float* b1,
                                      const void* w2_packed, const float* b2, const void* w3_packed,
                                      const float* b3, const void* w4_packed, const float* b4, void* out,
                                      lfd_stream_t stream);

/* The one-launch 'faster' stem writing the int8 map (k_stem2x only; the stem_int8 option): with y the fp16 value
 * lfd_stem_faster_fused_f16 stores for the same operands with the knob LFD_TUNE_STEM2X at its default of 1,
 *   out = clamp(rint((float)y * inv_scale), -127, 127), int8 NHWC [n, ceil(ceil(h/2)/2), ceil(ceil(w/2)/2), 64],
 * equal in every bit to that launch followed by lfd_quantize_nhwc_f16_i8 for finite y and finite inv_scale; a NaN becomes 0,
 * as it does there.  The fp16 map is not written.  LFD_TUNE_X2_ALN and LFD_TUNE_X2_STAGGER act as in the fp16 entry point;
 * LFD_TUNE_STEM2X does not (there is no int8 form of the older kernel).
 * in_format 1 (NHWC fp16) and 2 (NHWC uint8), channels == 64: everything else -- NCHW fp32 frames, 32-channel stems -- is
 * LFD_ERR_UNSUPPORTED (lfd_stem_faster_fused_i8_supported(in_format, channels) answers without launching).  out, the four
 * filters and the four biases: 16-byte aligned.  LFD_ERR_INVALID_ARGUMENT: a NULL pointer, a misaligned pointer, n / h / w < 1
 * -- checked on the host before any launch.  A refused call launches and writes nothing. */
LFD_API int lfd_stem_faster_fused_i8(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels,
                                     const void* w1_packed, const float* b1, const void* w2_packed, const float* b2,
                                     const void* w3_packed, const float* b3, const void* w4_packed, const float* b4,
                                     float inv_scale, void* out, lfd_stream_t stream);
LFD_API int lfd_stem_faster_fused_i8_supported(int32_t in_format, int32_t channels);

/* ------------------------------------------------------------------------------------------
 * Training-mode conv stack.  The reference trains through PyTorch autograd over
 * nn.Conv2d(bias=False) + nn.BatchNorm2d + ReLU (+ residual add) units (lfd_resnet.py:96-154 blocks,
 * :354-439 stem, :458-468 downsample; `loss.backward()` at optimizer_hook.py:28).  Here activations and
 * activation gradients are NHWC fp16 (gradients multiplied by a power-of-two loss scale; `inv_scale`
 * = 1/scale is applied where fp32 parameter gradients are written), statistics and parameter
 * gradients fp32.  A conv unit's forward is lfd_conv2d_nhwc_f16 (bias NULL-equivalent: zero bias, no
 * ReLU) -> lfd_bn_train_stats_f16 -> lfd_bn_train_apply_f16; its backward lfd_bn_train_bwd_f16 ->
 * lfd_conv_wgrad_nhwc_f16 + lfd_conv2d_nhwc_f16 on the transposed, tap-flipped weights (stride 2:
 * after lfd_zero_insert2_nhwc_f16).  channels: power of two in [8, 256].  Every reduction is per-block
 * partials + a fixed-order final stage (deterministic).  `workspace`: lfd_train_workspace_bytes().
 * Parameter-gradient outputs (dgamma, dbeta, dw) are `+=` when `accumulate` != 0 -- they can be the
 * zeroed .grad buffers themselves (autograd's AccumulateGrad semantics without a temporary + add per tensor).
 */
LFD_API size_t lfd_train_workspace_bytes(void);
/* nn.Conv2d.weight [cout, cin, ks, ks] fp32 -> the fp16 MFMA fragment order lfd_conv2d_nhwc_f16 consumes
 * (lfd_conv_packed_weight_halfs).  mode 0: the forward conv, rows >= rows_valid zero-filled (cout must already be the
 * padded row count, multiple of 32); mode 1: the data-gradient conv (channel roles swapped, taps flipped). */
LFD_API int lfd_pack_conv_weight_train_f16(const float* weight_oihw, int32_t cout, int32_t cin, int32_t ks, int32_t mode,
                                   int32_t rows_valid, void* packed, lfd_stream_t stream);
/* The same for many convs in one launch (the weights change every iteration: all forward packs at the start of the
 * forward, all data-gradient packs at the start of the backward).  `jobs_device`: table in device memory, sorted by
 * first_vec (= running sum of the jobs' output vectors of 8 halfs); fields as in lfd_pack_conv_weight_train_f16. */
typedef struct lfd_pack_job {
  const float* w;
  void* out;
  int32_t cout, cin, ks, mode, rows_valid, first_vec;
} lfd_pack_job_t;
LFD_API int lfd_pack_conv_weights_train_f16(const lfd_pack_job_t* jobs_device, int32_t njobs, int32_t total_vecs,
                                    lfd_stream_t stream);
/* batch statistics of y [pixels, channels]: stats[0..C) = mean, stats[C..2C) = 1/sqrt(biased var + eps)
 * (F.batch_norm training=True); running_mean / running_var (nullable) are updated with `momentum` and
 * the unbiased variance like nn.BatchNorm2d. */
LFD_API int lfd_bn_train_stats_f16(const void* y, int64_t pixels, int32_t channels, float eps, float momentum,
                           float* running_mean, float* running_var, void* workspace, size_t workspace_bytes,
                           float* stats, lfd_stream_t stream);
/* The conv in front of a train-mode BatchNorm and the batch statistics of its output in one pass (replaces
 * lfd_conv2d_nhwc_f16 -> lfd_bn_train_stats_f16 for a unit nn.Conv2d(bias=False) -> nn.BatchNorm2d, lfd_resnet.py:96-154,
 * :354-439, :458-468 in train mode): the conv kernel sums the fp16 values it stores and their squares per channel on the
 * way out, one row of partials per workgroup in `workspace`; the fp64 final pass is lfd_bn_train_stats_f16's.  `d->relu`
 * and `d->tail_cout` must be 0.  Shapes without such a kernel run the two calls it replaces.  `out`, `stats`,
 * running_mean / running_var as in the two calls. */
LFD_API int lfd_conv2d_bn_stats_nhwc_f16(const lfd_conv_desc_t* d, const void* in, void* out, const void* w_packed,
                                 const float* bias, const void* zeros, float eps, float momentum, float* running_mean,
                                 float* running_var, void* workspace, size_t workspace_bytes, float* stats,
                                 lfd_stream_t stream);
/* A 1x1 stride-1 conv unit whose INPUT is the activation of a train-mode BatchNorm + ReLU unit WITHOUT a residual
 * (lfd_resnet.py:376-413: the second conv of each stem pair): `y_in` is that unit's PRE-normalisation conv output and
 * (in_stats, in_gamma, in_beta) its batch statistics (lfd_bn_train_stats_f16 layout) and affine; the kernel normalises +
 * ReLUs its activation fragments on their way into the MFMA with lfd_bn_train_apply_f16's arithmetic (bit-identical to
 * applying first), so the producer's z tensor is never written or read.  Everything else as lfd_conv2d_bn_stats_nhwc_f16;
 * d->cin must be 64, d->ks = d->stride = 1.  The matching weight gradient: lfd_conv1x1_wgrad_partials_of_bn_relu_f16. */
LFD_API int lfd_conv1x1_of_bn_relu_bn_stats_nhwc_f16(const lfd_conv_desc_t* d, const void* y_in, const float* in_stats,
                                             const float* in_gamma, const float* in_beta, void* out, const void* w_packed,
                                             const float* bias, const void* zeros, float eps, float momentum,
                                             float* running_mean, float* running_var, void* workspace,
                                             size_t workspace_bytes, float* stats, lfd_stream_t stream);
/* z = relu?( gamma * (y - mean) * rstd + beta (+ residual) ) */
LFD_API int lfd_bn_train_apply_f16(const void* y, int64_t pixels, int32_t channels, const float* stats, const float* gamma,
                           const float* beta, const void* residual, int32_t relu, void* z, lfd_stream_t stream);
/* backward of the above: g = dz * [ReLU passed] (relu == 0: no ReLU; z given: mask = [z > 0]; z NULL: the mask is
 * recomputed from y as [gamma * xhat + beta > 0], only valid without a residual input), dgamma = inv_scale * sum g * xhat,
 * dbeta = inv_scale * sum g, dy = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)); g_out (nullable)
 * receives g, the gradient of the residual branch. */
LFD_API int lfd_bn_train_bwd_f16(const void* dz, const void* y, const void* z, int32_t relu, int64_t pixels, int32_t channels,
                         const float* stats, const float* gamma, const float* beta, float inv_scale,
                         int32_t accumulate, void* workspace,
                         size_t workspace_bytes, float* dgamma, float* dbeta, void* dy, void* g_out,
                         lfd_stream_t stream);
/* GroupNorm of the head towers in training (nn.GroupNorm(groups, channels) + ReLU, lfd_head.py:97-105), groups of
 * exactly 8 channels (128 / 16): stats[img][0][g] = mean, [1][g] = rstd over hw x 8 elements; apply; backward
 * (dgamma / dbeta are `+=` when accumulate != 0: the towers are shared by all pyramid levels, lfd_head.py:67-82). */
LFD_API int lfd_gn_train_stats_f16(const void* y, int32_t n, int64_t hw, int32_t channels, int32_t groups, float eps,
                           void* workspace, size_t workspace_bytes, float* stats, lfd_stream_t stream);
LFD_API int lfd_gn_train_apply_f16(const void* y, int32_t n, int64_t hw, int32_t channels, int32_t groups, const float* stats,
                           const float* gamma, const float* beta, int32_t relu, void* z, lfd_stream_t stream);
/* lfd_gn_train_stats_f16 + lfd_gn_train_apply_f16 in two launches instead of three: the apply pass adds the per-block partial
 * sums of its image itself (same fp64 arithmetic; `stats` is an OUTPUT here, written for the backward pass). */
LFD_API int lfd_gn_train_stats_apply_f16(const void* y, int32_t n, int64_t hw, int32_t channels, int32_t groups, float eps,
                                 const float* gamma, const float* beta, int32_t relu, void* workspace, size_t workspace_bytes,
                                 float* stats, void* z, lfd_stream_t stream);
LFD_API int lfd_gn_train_bwd_f16(const void* dz, const void* y, const void* z, int32_t n, int64_t hw, int32_t channels,
                         int32_t groups, const float* stats, const float* gamma, float inv_scale, int32_t accumulate,
                         void* workspace, size_t workspace_bytes, float* dgamma, float* dbeta, void* dy,
                         lfd_stream_t stream);
/* out[n, 2i, 2j, :] = in[n, i, j, :], zero elsewhere; ho in {2*hi-1, 2*hi}, wo likewise */
LFD_API int lfd_zero_insert2_nhwc_f16(const void* in, int32_t n, int32_t hi, int32_t wi, int32_t channels, int32_t ho,
                              int32_t wo, void* out, lfd_stream_t stream);
/* Data gradient of a 3x3 stride-2 pad-1 convolution, 64 -> 64 channels, WITHOUT the zero-inserted tensor:
 *   dx [n, h, w, 64] = conv3x3_s1(zero_insert2(dy), w)  (+ residual)   computed per output parity (1 / 2 / 2 / 4 taps),
 * dy [n, (h-1)/2+1, (w-1)/2+1, 64]; w_packed = the data-gradient pack of the conv's weight (lfd_pack_conv_weight_train_f16 with
 * mode 1: roles swapped, taps flipped -- the fragments lfd_conv2d_nhwc_f16 would consume on the zero-inserted tensor);
 * residual (nullable): the gradient already collected for the same activation, added before the fp16 rounding.  Bit-identical
 * to lfd_zero_insert2_nhwc_f16 + lfd_conv2d_nhwc_f16 (csrc/dgrad_s2.hip). */
LFD_API int lfd_conv3x3s2_dgrad_nhwc_f16(int32_t n, int32_t h, int32_t w, const void* dy, void* dx, const void* w_packed,
                                         const void* residual, lfd_stream_t stream);
/* dW [cout, cin, ks, ks] fp32 (OIHW, the nn.Conv2d.weight layout) = inv_scale * sum over pixels of
 * dy (x) x for a conv with pad ks/2; x [n,h,w,cin], dy [n,ho,wo,cout]; cin, cout multiples of 8, <= 128. */
LFD_API int lfd_conv_wgrad_nhwc_f16(const void* x, const void* dy, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout,
                            int32_t ks, int32_t stride, float inv_scale, int32_t accumulate, void* workspace,
                            size_t workspace_bytes, float* dw, lfd_stream_t stream);
/* The LEVEL-CONCATENATED form of the head's training passes (round 4).  The reference's head applies the SAME towers to every
 * pyramid level, one tensor per level (lfd_head.py:164-185); the training schedule keeps the levels of an image back to back in
 * one tensor [n, P, c] (P = points of all levels, the layout LFD.forward returns, lfd.py:526-542), so that a shared 1x1 conv, its
 * weight gradient and its data gradient are ONE launch over all levels instead of one per level:
 *   lfd_bn_train_apply_into_f16   a level's neck unit writes its normalised output into rows [point0, point0 + hw) of every image;
 *   lfd_bn_train_bwd_from_f16     ... and reads its output gradient from there (no residual input; ReLU mask recomputed from y);
 *   lfd_gn_train_*_seg_f16        GroupNorm with statistics per (image, segment): nseg segments of seg_hw[] pixels per image,
 *                                 stats [n * nseg][2][groups] (virtual image = img * nseg + segment);
 *   lfd_head_out_*_concat_f16     the glue kernels below with y / dy = the concatenated conv output [n, P, 64]. */
LFD_API int lfd_bn_train_apply_into_f16(const void* y, int32_t n, int64_t hw, int32_t channels, const float* stats, const float* gamma,
                                const float* beta, int32_t relu, void* z_concat, int64_t points_total, int64_t point0,
                                lfd_stream_t stream);
/* The forward counterpart: the convs of several independent units leave their statistics rows behind
 * (lfd_conv2d_bn_partials_nhwc_f16: lfd_conv2d_bn_stats_nhwc_f16 without its final pass, rows in the caller's buffer of at
 * least 512 x 2 x cout floats, *nrows = how many), then ONE call finishes all of them: the per-channel finals (mean, rstd,
 * running statistics) of every level in one launch, the apply passes into the level-concatenated tensor in another.  Values
 * bit-identical to lfd_conv2d_bn_stats_nhwc_f16 + lfd_bn_train_apply_into_f16 per level. */
LFD_API int lfd_conv2d_bn_partials_nhwc_f16(const lfd_conv_desc_t* d, const void* in, void* out, const void* w_packed, const float* bias,
                                    const void* zeros, float* rows, size_t rows_bytes, int32_t* nrows, lfd_stream_t stream);
typedef struct {
  const void* y;           /* [n, hw, channels] fp16 */
  const float* rows;       /* statistics rows of the conv that produced y */
  float* running_mean;     /* nullable (both or none) */
  float* running_var;
  float* stats;            /* out: [2][channels] */
  const float* gamma;
  const float* beta;
  int64_t hw, point0;
  int32_t channels, nrows;
  float eps, momentum;
} lfd_bn_fwd_level_t;
LFD_API int lfd_bn_train_finish_into_levels_f16(const lfd_bn_fwd_level_t* levels, int32_t nlevels, int32_t n, int32_t relu,
                                        void* z_concat, int64_t points_total, lfd_stream_t stream);
/* lfd_bn_train_bwd_from_f16 for SEVERAL levels (units of the same batch, independent of each other: the neck units of the pyramid
 * levels) in three launches instead of three per level; values bit-identical to the per-level calls.  `levels`: host array. */
typedef struct {
  const void* y;          /* the level's pre-normalisation output [n, hw, channels] fp16 */
  void* dy;               /* out: [n, hw, channels] fp16 */
  const float* stats;     /* [2][channels] */
  const float* gamma;
  const float* beta;
  float* dgamma;          /* [channels], (+)= */
  float* dbeta;
  int64_t hw, point0;     /* pixels per image; first point of the level inside an image of dz_concat */
  int32_t channels;
  int32_t reserved_;
} lfd_bn_bwd_level_t;
LFD_API int lfd_bn_train_bwd_from_levels_f16(const void* dz_concat, int64_t points_total, const lfd_bn_bwd_level_t* levels,
                                     int32_t nlevels, int32_t relu, int32_t n, float inv_scale, int32_t accumulate,
                                     void* workspace, size_t workspace_bytes, lfd_stream_t stream);
LFD_API int lfd_bn_train_bwd_from_f16(const void* dz_concat, int64_t points_total, int64_t point0, const void* y, int32_t relu, int32_t n,
                              int64_t hw, int32_t channels, const float* stats, const float* gamma, const float* beta,
                              float inv_scale, int32_t accumulate, void* workspace, size_t workspace_bytes, float* dgamma,
                              float* dbeta, void* dy, lfd_stream_t stream);
LFD_API int lfd_gn_train_stats_apply_seg_f16(const void* y, int32_t n, int32_t nseg, const int64_t* seg_hw, int32_t channels,
                                     int32_t groups, float eps, const float* gamma, const float* beta, int32_t relu,
                                     void* workspace, size_t workspace_bytes, float* stats, void* z, lfd_stream_t stream);
LFD_API int lfd_gn_train_bwd_seg_f16(const void* dz, const void* y, const void* z, int32_t n, int32_t nseg, const int64_t* seg_hw,
                             int32_t channels, int32_t groups, const float* stats, const float* gamma, float inv_scale,
                             int32_t accumulate, void* workspace, size_t workspace_bytes, float* dgamma, float* dbeta, void* dy,
                             lfd_stream_t stream);
/* The same weight gradient in two stages for a schedule that defers the final sums (round 4): every conv's k_wgrad writes
 * its per-workgroup partial sums into ITS OWN buffer (`partials`: lfd_conv_wgrad_partial_rows() x blocks x ks*ks x 64 x 64
 * floats, blocks = ceil(cout/64) * ceil(cin/64)), and ONE lfd_wgrad_final_batched_f32 launch after the last of them turns all
 * buffers into dW tensors -- the 49 dependent final launches of a WIDERFACE_LFD_S iteration become one, and the partial
 * launches may run on another stream than the data-gradient chain.  Job table in device memory: head jobs (first_block >= 0,
 * = running sum of the head jobs' nblk * taps * 32 blocks) own output blocks; `next` chains further partial sets of the same dW
 * (a conv shared by the pyramid levels, lfd_head.py:67-82; chained jobs have first_block = -1 and the head job's nblk / taps),
 * summed after the head's rows in chain order, fp64, one rounding.  Rows [co_lo, co_hi) of the conv go to dw rows
 * [0, co_hi - co_lo): the padded per-level output conv writes its classification and regression rows into two tensors
 * through two head jobs over the same partials.  dW (+)= inv_scale * sum. */
typedef struct lfd_wgrad_job {
  const float* partials;
  float* dw;
  int32_t nwg, nblk, cin, cout, taps;
  int32_t co_lo, co_hi;
  int32_t first_block, next, accumulate;
  float inv_scale;
} lfd_wgrad_job_t;
LFD_API int32_t lfd_conv_wgrad_partial_rows(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ks, int32_t stride);
LFD_API int lfd_conv_wgrad_partials_nhwc_f16(const void* x, const void* dy, int32_t n, int32_t h, int32_t w, int32_t cin,
                                             int32_t cout, int32_t ks, int32_t stride, float* partials, size_t partials_bytes,
                                             lfd_stream_t stream);
/* lfd_conv_wgrad_partials_nhwc_f16 for a 1x1 stride-1 conv whose operand x = relu(BatchNorm(y_in)) was never stored (see
 * lfd_conv1x1_of_bn_relu_bn_stats_nhwc_f16): the tile loader re-forms it from y_in.  Same partial rows / final pass. */
LFD_API int lfd_conv1x1_wgrad_partials_of_bn_relu_f16(const void* y_in, const float* in_stats, const float* in_gamma,
                                              const float* in_beta, const void* dy, int32_t n, int32_t h, int32_t w,
                                              int32_t cin, int32_t cout, float* partials, size_t partials_bytes,
                                              lfd_stream_t stream);
LFD_API int lfd_wgrad_final_batched_f32(const lfd_wgrad_job_t* jobs_device, int32_t njobs, int32_t total_blocks,
                                        lfd_stream_t stream);
/* dst[i] (+)= sum over r < nrows of src[r * row_stride + i], i < count, fp64 in row order; one block per job: the private
 * per-level copies of small shared parameter gradients (GroupNorm weight / bias of shared towers, output-conv biases)
 * after the pyramid levels ran on their own streams. */
typedef struct lfd_rowsum_job {
  const float* src;
  float* dst;
  int32_t nrows, row_stride, count, accumulate;
} lfd_rowsum_job_t;
LFD_API int lfd_rows_sum_batched_f32(const lfd_rowsum_job_t* jobs_device, int32_t njobs, lfd_stream_t stream);
/* The glue around the head's per-level OUTPUT convs in a training iteration (csrc/head_out.hip).  The reference's head ends,
 * per level, in a classification and a regression conv with fp32 outputs, the regression one through a learnable per-level
 * Scale (lfd_head.py:157-185); LFD.forward concatenates the levels along the point axis (lfd.py:526-542).  The training
 * engine runs a level's convs as ONE 1x1 conv padded to 64 output rows; `y` [n, hw, 64] fp16 is its output, a segment is
 * the row range [row0, row0 + channels) of one of the convs.
 *   lfd_head_out_split_f16: out[img, point0 + p, j] = float(y[img, p, row0 + j]) (* *scale) for every segment -- `out` is the
 *     level-concatenated [n, points_total, channels] fp32 tensor.
 *   lfd_head_out_grad_f16: from grad (same layout as out) writes dy [n, hw, 64] fp16 = grad (* *scale) * loss_scale (other rows
 *     zero) and ACCUMULATES dbias[j] += sum grad (* *scale), *dscale += sum grad * float(y) (both nullable) through per-block
 *     partials in `workspace` (>= 512 KB) and one fixed-order fp64 final launch: what autograd computes for
 *     conv bias / Scale, as 2 launches instead of ~20 per level.
 * `y` and `dy` must be 16-byte aligned (forward and backward move a pixel's line in 16-byte pieces); a misaligned pointer
 * returns LFD_ERR_INVALID_ARGUMENT. */
typedef struct lfd_head_out_seg {
  float* out;          /* split: destination */
  const float* grad;   /* grad: source */
  float* dbias;        /* grad: [channels], += (nullable) */
  const float* scale;  /* device scalar (nullable: no Scale) */
  float* dscale;       /* grad: device scalar, += (nullable) */
  int32_t channels, row0;
} lfd_head_out_seg_t;
LFD_API int lfd_head_out_split_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                           const lfd_head_out_seg_t* segs, int32_t nsegs, lfd_stream_t stream);
LFD_API int lfd_head_out_grad_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                          const lfd_head_out_seg_t* segs, int32_t nsegs, float loss_scale, void* dy, void* workspace,
                          size_t workspace_bytes, lfd_stream_t stream);
LFD_API int lfd_head_out_split_concat_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                  const lfd_head_out_seg_t* segs, int32_t nsegs, lfd_stream_t stream);
LFD_API int lfd_head_out_grad_concat_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                 const lfd_head_out_seg_t* segs, int32_t nsegs, float loss_scale, void* dy_concat, void* workspace,
                                 size_t workspace_bytes, lfd_stream_t stream);

/* ... and ALL pyramid levels of one (shared) output conv in one launch each (round 4): the per-level calls of the two `_concat`
 * entry points above, with the levels as blockIdx.y -- every level keeps its own block count and the final stage adds the levels
 * in level order, so outputs, dy, dbias and dscale are those of the per-level call sequence, bit for bit.  `levels`: host array. */
typedef struct {
  int32_t hw;                      /* pixels per image of the level */
  int32_t nsegs;
  int64_t point0;                  /* first point of the level inside an image of the concatenated tensors */
  lfd_head_out_seg_t segs[2];
} lfd_head_out_level_t;
LFD_API int lfd_head_out_split_levels_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                  int32_t nlevels, lfd_stream_t stream);
LFD_API int lfd_head_out_grad_levels_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                 int32_t nlevels, float loss_scale, void* dy_concat, void* workspace, size_t workspace_bytes,
                                 lfd_stream_t stream);

/* The six entry points above for an output conv padded to `rows` output rows: `rows` is 64 or 128, the two instantiations of
 * the one row-width-templated implementation in csrc/head_out.hip; anything else returns LFD_ERR_INVALID_ARGUMENT.  rows == 64
 * runs the kernels of the entry point above of the same name; rows == 128 serves heads whose level needs more than 64 rows (a
 * merged head with 61..124 class channels + 4 regression rows, separate towers with up to 128 class channels): `y` / `dy` are
 * [n, hw, 128] (`_concat` / `_levels`: [n, points_total, 128]) fp16, 16-byte aligned as above, a segment must satisfy
 * row0 + channels <= 128, and n * hw * 128 < 2^31.  Same values as the 64-row kernels compute for the same segments: out and dy
 * are single roundings of the fp32 products, rows of dy outside every segment are zero, dbias / dscale accumulate through
 * per-block partials and one fixed-order fp64 final launch.  `workspace` of the 128-row gradient entry points: >= 1 MB (1024
 * blocks x 2 x 128 floats), `_levels`: >= nlevels x 1 MB; lfd_train_workspace_bytes() covers both. */
LFD_API int lfd_head_out_split_w_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                             const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, lfd_stream_t stream);
LFD_API int lfd_head_out_grad_w_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                            const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, float loss_scale, void* dy,
                            void* workspace, size_t workspace_bytes, lfd_stream_t stream);
LFD_API int lfd_head_out_split_concat_w_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                    const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, lfd_stream_t stream);
LFD_API int lfd_head_out_grad_concat_w_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                   const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, float loss_scale, void* dy_concat,
                                   void* workspace, size_t workspace_bytes, lfd_stream_t stream);
LFD_API int lfd_head_out_split_levels_w_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                    int32_t nlevels, int32_t rows, lfd_stream_t stream);
LFD_API int lfd_head_out_grad_levels_w_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                   int32_t nlevels, int32_t rows, float loss_scale, void* dy_concat, void* workspace,
                                   size_t workspace_bytes, lfd_stream_t stream);

/* The glue around FCOSHead's output convs in a training iteration (csrc/fcos_out.hip), all pyramid levels in one launch.
 * Replaces, forward, fcos_head.py:140-150 (`exp(Scale_i(regression conv))`, the classification / centerness outputs) and
 * fcos.py:414-449 (permute + reshape + concatenation of the levels along the point axis), and, backward, what autograd runs for
 * them.  The engine runs a level's three 3x3 convs as TWO convs padded to `rows` (32 | 64) output rows with fp32 outputs
 * (lfd_conv2d_nhwc_f16_acc32): raw_cls [n, hw, rows] holds classification in rows [0, C) and centerness in row C, raw_reg
 * [n, hw, rows] the regression rows [0, 4); the other rows are zero.
 *   lfd_fcos_out_pack_levels_f32: cls[img, point0 + p, c] = raw_cls[img, p, c], ctr[img, point0 + p, 0] = raw_cls[img, p, C],
 *     reg[img, point0 + p, k] = expf(raw_reg[img, p, k] * *scale) -- the bits lfd_pack_level_outputs_f32 gives on the same raw
 *     values.  cls [n, points_total, C], reg [n, points_total, 4], ctr [n, points_total, 1] fp32; every element of a level's
 *     point range is written.
 *   lfd_fcos_out_grad_levels_f32: from dcls / dreg / dctr (layouts of cls / reg / ctr), the stored `reg` and raw_reg writes
 *     dy_cls = d * loss_scale and dy_reg = dreg * reg * *scale * loss_scale [n, hw, rows] fp16 (one fp16 rounding of the
 *     correctly rounded fp32 value; rows outside the segments ZERO) and ACCUMULATES dbias_cls[c] += sum dcls,
 *     dbias_ctr[0] += sum dctr, dbias_reg[k] += sum dreg * reg * *scale over ALL levels (one rounding of the fp64 total) and, per
 *     level, *dscale += sum_k sum dreg * reg * raw_reg, through per-block fp32 partials in `workspace`
 *     (lfd_fcos_out_grad_workspace_bytes; lfd_train_workspace_bytes() covers it) and one fixed-order fp64 final launch: no
 *     atomics, equal bits run after run.
 * `levels`: host array.  raw_*, dy_*, reg, dreg, workspace: 16-byte aligned.  LFD_ERR_INVALID_ARGUMENT: a null / misaligned
 * pointer, rows not 32 | 64, num_classes + 1 > rows, nlevels > LFD_MAX_LEVELS, a point range outside points_total;
 * LFD_ERR_UNSUPPORTED: n * hw * rows >= 2^31 (32-bit indices); LFD_ERR_WORKSPACE_TOO_SMALL. */
typedef struct lfd_fcos_out_level {
  const float* raw_cls;  /* pack: [n, hw, rows] fp32 (grad: unused, nullable) */
  const float* raw_reg;  /* [n, hw, rows] fp32 */
  const float* scale;    /* device scalar: the level's Scale */
  float* dscale;         /* grad: device scalar, += */
  void* dy_cls;          /* grad: [n, hw, rows] fp16 */
  void* dy_reg;          /* grad: [n, hw, rows] fp16 */
  int32_t hw;            /* pixels per image of the level */
  int32_t reserved;
  int64_t point0;        /* first point of the level inside an image of the concatenated tensors */
} lfd_fcos_out_level_t;
LFD_API size_t lfd_fcos_out_grad_workspace_bytes(int32_t nlevels, int32_t rows);
LFD_API int lfd_fcos_out_pack_levels_f32(const lfd_fcos_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows,
                                         int32_t num_classes, int64_t points_total, float* cls, float* reg, float* ctr,
                                         lfd_stream_t stream);
LFD_API int lfd_fcos_out_grad_levels_f32(const lfd_fcos_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows,
                                         int32_t num_classes, int64_t points_total, const float* dcls, const float* dreg,
                                         const float* dctr, const float* reg, float loss_scale, float* dbias_cls, float* dbias_ctr,
                                         float* dbias_reg, void* workspace, size_t workspace_bytes, lfd_stream_t stream);

/* The glue around LFDHead's output convs with fp32 logits in a training iteration (csrc/lfd_out.hip), all pyramid levels and
 * both convs of a level in one launch.  Replaces, forward, lfd_head.py:157-185 (the classification conv's output, the regression
 * conv's output through the level's Scale) and lfd.py:526-542 (permute + reshape + concatenation of the levels along the point
 * axis), and, backward, what autograd runs for them.  The detector node runs a level's two 1x1 convs as ONE conv (both read the
 * same activation) or TWO (separate towers) padded to `rows` (64 | 128) output rows with fp32 outputs
 * (lfd_conv2d_nhwc_f16_acc32): `raw` [n, hw, rows].  A segment is the row range [row0, row0 + channels) of one of the
 * reference's convs inside a padded conv, kind 0 = classification (channels == cls_channels), 1 = regression (channels == 4); a
 * level has exactly one of each.
 *   lfd_lfdhead_out_pack_levels_f32: cls[img, point0 + p, j] = raw[img, p, row0 + j] (a copy) and reg[img, point0 + p, k] =
 *     raw[img, p, row0 + k] * *scale (one fp32 multiply; a copy when scale is null).  cls [n, points_total, cls_channels], reg
 *     [n, points_total, 4] fp32; every element of a level's point range is written.
 *   lfd_lfdhead_out_grad_levels_f32: from dcls / dreg (layouts of cls / reg) writes every conv's dy [n, hw, rows] fp16 =
 *     dcls * loss_scale and dreg * *scale * loss_scale (the product formed in fp64, rounded to fp32 once, then to fp16 once; rows
 *     outside the segments ZERO) and ACCUMULATES dbias[j] += sum dcls | sum dreg * *scale -- the sums of consecutive levels whose
 *     segments name the same dbias (a head shared by the levels) reach it as one rounding of their fp64 total; a head with its own
 *     convs per level names one target per level -- and, per level with a Scale, *dscale += sum_k sum dreg * raw, through
 *     per-block fp32 partials in `workspace` (lfd_lfdhead_out_grad_workspace_bytes; lfd_train_workspace_bytes() covers it) and
 *     one fixed-order fp64 final launch: no atomics, equal bits run after run.  A dbias element belongs to one (conv position, row)
 *     of the levels that name it.
 * `levels`: host array.  raw, dy, reg, dreg, workspace: 16-byte aligned (cls / dcls move as float4 where they are).
 * LFD_ERR_INVALID_ARGUMENT: a null / misaligned pointer (dscale must be given iff scale is), rows not 64 | 128, nconvs / nsegs
 * outside 1..2, a segment past `rows`, overlapping segments, channels that are not cls_channels / 4, a level without exactly one
 * segment of each kind, nlevels > LFD_MAX_LEVELS, a point range outside points_total; LFD_ERR_UNSUPPORTED: n * hw * rows >= 2^31
 * (32-bit indices); LFD_ERR_WORKSPACE_TOO_SMALL.  Nothing is launched when a status code is returned. */
typedef struct lfd_lfdhead_out_seg {
  float* dbias;          /* grad: [channels] fp32, += (pack: unused) */
  int32_t row0;          /* first row of the segment inside the padded conv */
  int32_t channels;
  int32_t kind;          /* 0: classification, 1: regression */
  int32_t reserved;
} lfd_lfdhead_out_seg_t;
typedef struct lfd_lfdhead_out_conv {
  const float* raw;      /* [n, hw, rows] fp32: the padded conv's output (grad: read, and required, only where the conv holds
                          * the regression rows of a level with a Scale) */
  void* dy;              /* grad: [n, hw, rows] fp16 (pack: unused) */
  int32_t nsegs;         /* 1 | 2 */
  int32_t reserved;
  lfd_lfdhead_out_seg_t segs[2];
} lfd_lfdhead_out_conv_t;
typedef struct lfd_lfdhead_out_level {
  const float* scale;    /* device scalar: the level's Scale (null: the head has none) */
  float* dscale;         /* grad: device scalar, += (null iff scale is) */
  int32_t hw;            /* pixels per image of the level */
  int32_t nconvs;        /* 1 | 2 */
  int64_t point0;        /* first point of the level inside an image of the concatenated tensors */
  lfd_lfdhead_out_conv_t convs[2];
} lfd_lfdhead_out_level_t;
LFD_API size_t lfd_lfdhead_out_grad_workspace_bytes(int32_t nlevels, int32_t rows);
LFD_API int lfd_lfdhead_out_pack_levels_f32(const lfd_lfdhead_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows,
                                            int32_t cls_channels, int64_t points_total, float* cls, float* reg,
                                            lfd_stream_t stream);
LFD_API int lfd_lfdhead_out_grad_levels_f32(const lfd_lfdhead_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows,
                                            int32_t cls_channels, int64_t points_total, const float* dcls, const float* dreg,
                                            float loss_scale, void* workspace, size_t workspace_bytes, lfd_stream_t stream);

/* first stem conv (3 -> channels, 3x3 stride 2 pad 1, lfd_resnet.py:358,:378) on the NCHW fp32 image batch:
 * forward -> y NHWC fp16 (pre-norm), and its weight gradient (OIHW fp32); channels in {32, 64} */
LFD_API int lfd_stem_conv0_train_fwd(const float* x_nchw, int32_t n, int32_t h, int32_t w, int32_t channels,
                             const float* weight_oihw, void* y, lfd_stream_t stream);
/* the same conv with the batch statistics of its train-mode BatchNorm (lfd_resnet.py:358-359) taken from the values on
 * their way to memory (64 channels; 32 channels: conv, then lfd_bn_train_stats_f16); stats / running_* / workspace as in
 * lfd_bn_train_stats_f16 */
LFD_API int lfd_stem_conv0_train_fwd_bn_stats(const float* x_nchw, int32_t n, int32_t h, int32_t w, int32_t channels,
                                      const float* weight_oihw, void* y, float eps, float momentum, float* running_mean,
                                      float* running_var, void* workspace, size_t workspace_bytes, float* stats,
                                      lfd_stream_t stream);
LFD_API int lfd_stem_conv0_wgrad(const float* x_nchw, const void* dy, int32_t n, int32_t h, int32_t w, int32_t channels,
                         float inv_scale, int32_t accumulate, void* workspace, size_t workspace_bytes, float* dw, lfd_stream_t stream);
/* The backward of the FIRST conv unit (Conv2d(3, 64, 3, 2, 1, bias=False) -> train-mode BatchNorm2d -> ReLU, lfd_resnet.py:358-366)
 * without materialising dL/dy: BatchNorm's sums (dgamma, dbeta +=) and the conv's weight gradient computed straight from dz = dL/dz
 * of the unit's output and its stored pre-norm output y -- the unit has no data gradient, so its dy has no other consumer.  The
 * values are those of lfd_bn_train_bwd_f16 (ReLU mask recomputed from y) followed by lfd_stem_conv0_wgrad, bit for bit. */
LFD_API int lfd_stem_conv0_bn_bwd_wgrad(const float* x_nchw, const void* dz, const void* y, int32_t n, int32_t h, int32_t w,
                                int32_t channels, const float* stats, const float* gamma, const float* beta, float inv_scale,
                                int32_t accumulate, void* workspace, size_t workspace_bytes, float* dgamma, float* dbeta, float* dw,
                                lfd_stream_t stream);

/* BatchNorm's backward sums in the epilogue of the data-gradient conv that produces dz (round 4; the stem pairs,
 * lfd_resnet.py:376-413): a unit Conv -> train-mode BatchNorm2d -> ReLU (no residual) whose activation feeds exactly one 1x1
 * stride-1 conv gets its dz = dL/d(activation) from that conv's data gradient -- a 1x1 conv over dy with the transposed
 * weights.  lfd_conv1x1_dgrad_bn_bwd_sums_nhwc_f16 runs that conv (desc: cin = cout = 64, ks = stride = 1, relu = 0; bias:
 * 64 zeros) and, while copying dz out, adds sum g and sum g * xhat per channel (g = dz * [gamma * xhat + beta > 0], the
 * arithmetic of lfd_bn_train_bwd_f16's first pass on the fp16 values it stores) into one row per workgroup in `workspace`;
 * *sum_rows (host) receives the row count.  The unit's backward then skips its own pass over (dz, y):
 *   lfd_bn_train_bwd_rows_f16           the final + apply stages of lfd_bn_train_bwd_f16 (ReLU mask recomputed from y, no g output)
 *   lfd_stem_conv0_bn_bwd_wgrad_rows    lfd_stem_conv0_bn_bwd_wgrad without its sums pass (sum_rows = 0: with it)
 * with the SAME workspace and no other workspace user in between.  Values equal the unfused calls up to the order of the
 * fp32 partial sums. */
LFD_API int lfd_conv1x1_dgrad_bn_bwd_sums_nhwc_f16(const lfd_conv_desc_t* d, const void* dy, void* dz, const void* w_packed,
                                           const float* bias, const void* zeros, const void* y_unit, const float* unit_stats,
                                           const float* unit_gamma, const float* unit_beta, void* workspace,
                                           size_t workspace_bytes, int32_t* sum_rows, lfd_stream_t stream);
LFD_API int lfd_bn_train_bwd_rows_f16(const void* dz, const void* y, int64_t pixels, int32_t channels, const float* stats,
                              const float* gamma, const float* beta, float inv_scale, int32_t accumulate, int32_t sum_rows,
                              void* workspace, size_t workspace_bytes, float* dgamma, float* dbeta, void* dy, lfd_stream_t stream);
LFD_API int lfd_stem_conv0_bn_bwd_wgrad_rows(const float* x_nchw, const void* dz, const void* y, int32_t n, int32_t h, int32_t w,
                                     int32_t channels, const float* stats, const float* gamma, const float* beta, float inv_scale,
                                     int32_t accumulate, int32_t sum_rows, void* workspace, size_t workspace_bytes, float* dgamma,
                                     float* dbeta, float* dw, lfd_stream_t stream);

/* The first stem conv of a ONE-channel (grayscale) model in training (csrc/stem_gray_train.hip): Conv2d(1, channels, 3, 2, 1,
 * bias=False) -> train-mode BatchNorm2d -> ReLU, lfd_resnet.py:354-439 with input_channels = 1 (lfd_resnet.py:358 'fast' stem,
 * :378 'faster' stem).  The gray twins of the four RGB entry points above, same arguments and numerics: x_nchw is fp32 [n,1,h,w],
 * weight_oihw / dw fp32 [channels,1,3,3], y / dy / dz NHWC fp16 [n,(h+1)/2,(w+1)/2,channels] (16-byte aligned), channels in
 * {32, 64}; image values rounded to fp16 for the MFMA, fp32 accumulation, dw and dgamma / dbeta unscaled (x inv_scale),
 * accumulate: += instead of =; every reduction in a fixed order (deterministic).
 *   lfd_stem_gray_train_fwd            y = conv(x, W), pre-norm
 *   lfd_stem_gray_train_fwd_bn_stats   the same y, bit for bit, + the batch statistics as lfd_stem_conv0_train_fwd_bn_stats
 *   lfd_stem_gray_wgrad                dw (+)= inv_scale * sum_px dy[px][co] * patch[px][t]
 *   lfd_stem_gray_bn_bwd_wgrad_rows    BatchNorm backward (ReLU mask recomputed from y) + dw without a dy tensor: the values of
 *                                      lfd_bn_train_bwd_f16 followed by lfd_stem_gray_wgrad, bit for bit; sum_rows as
 *                                      lfd_stem_conv0_bn_bwd_wgrad_rows (0: with the sums pass)
 * LFD_ERR_INVALID_ARGUMENT for null or misaligned pointers, channels not in {32, 64}, n, h or w < 1, sum_rows outside 0..1024;
 * LFD_ERR_UNSUPPORTED for an image or output map of 2^31 elements or more; LFD_ERR_WORKSPACE_TOO_SMALL below
 * lfd_train_workspace_bytes().  Nothing is launched when a status code is returned. */
LFD_API int lfd_stem_gray_train_fwd(const float* x_nchw, int32_t n, int32_t h, int32_t w, int32_t channels,
                                    const float* weight_oihw, void* y, lfd_stream_t stream);
LFD_API int lfd_stem_gray_train_fwd_bn_stats(const float* x_nchw, int32_t n, int32_t h, int32_t w, int32_t channels,
                                             const float* weight_oihw, void* y, float eps, float momentum, float* running_mean,
                                             float* running_var, void* workspace, size_t workspace_bytes, float* stats,
                                             lfd_stream_t stream);
LFD_API int lfd_stem_gray_wgrad(const float* x_nchw, const void* dy, int32_t n, int32_t h, int32_t w, int32_t channels,
                                float inv_scale, int32_t accumulate, void* workspace, size_t workspace_bytes, float* dw,
                                lfd_stream_t stream);
LFD_API int lfd_stem_gray_bn_bwd_wgrad_rows(const float* x_nchw, const void* dz, const void* y, int32_t n, int32_t h, int32_t w,
                                            int32_t channels, const float* stats, const float* gamma, const float* beta,
                                            float inv_scale, int32_t accumulate, int32_t sum_rows, void* workspace,
                                            size_t workspace_bytes, float* dgamma, float* dbeta, float* dw, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Neck + head of ALL pyramid levels.  Replaces SimpleNeck.forward (simple_neck.py:67-74),
 * LFDHead.forward (lfd_head.py:164-185: GroupNorm towers + cls/reg convs + Scale) and the
 * NCHW -> [N,P,C] permute/concat of LFD.forward (lfd.py:526-542): writes the fp32 cls / reg rows of
 * every level directly at its point offset of the level-concatenated outputs.
 * GroupNorm statistics are obtained by recomputing the chain (pass 1, 2) -- see csrc/head.hip.
 *   pass 1: per-tile stats of tower conv1 -> `partial`;  lfd_groupnorm_finalize -> ab1
 *   pass 2: per-tile stats of tower conv2 -> `partial`;  lfd_groupnorm_finalize -> ab2
 *   pass 3: outputs.
 * For a BatchNorm / no-norm head, skip passes 1-2 and pass the folded (scale, shift) as ab1/ab2.
 * One call = one tower (merged cls+reg tower, or the cls / reg tower of an unmerged head). */
typedef struct lfd_head_desc {
  int32_t n;                                  /* images */
  int32_t num_levels;
  int32_t level_hw[LFD_MAX_LEVELS];           /* pixels (h*w) per level */
  int32_t level_cin[LFD_MAX_LEVELS];          /* backbone tap channels per level: 64 | 128 */
  int32_t level_point_offset[LFD_MAX_LEVELS]; /* first point of each level in [0, P) */
  int32_t head_channels;                      /* 128 */
  int32_t num_groups;                         /* GroupNorm groups (16) */
  int32_t total_points;                       /* P */
  int32_t cls_channels;                       /* C' (row length of out_cls) */
  int32_t final_reg_rows;                     /* final conv rows [0, reg_rows) -> reg: 0 or 4 */
  int32_t final_cls_rows;                     /* ... followed by cls_rows rows -> cls (output pass: reg+cls <= 64 through
                                               * lfd_head_forward_f16, 64 < reg+cls <= 128 through lfd_head_forward_wide_f16) */
} lfd_head_desc_t;

typedef struct lfd_head_level_ptrs {
  const void* x;           /* [n, hw, cin] fp16 backbone tap (NHWC) */
  const void* wn_packed;   /* neck conv1x1 (BN folded), packed */
  const float* bn;         /* neck bias [128] */
  const void* w1_packed;   /* tower conv 1, packed */
  const void* w2_packed;   /* tower conv 2, packed */
  const void* wf_packed;   /* final conv (rows padded to a multiple of 32), packed */
  const float* bf;         /* final bias */
  const float* scale;      /* per-level Scale (device scalar) or NULL */
  /* optional scratch, LFD_HEAD_FOLDED_HALFS halfs per image each ([n] images): tower conv 1 / 2 with the GroupNorm scale
   * of (level, image) folded into the rows and the shift as a bias fragment, in the kernel's register layout -- written
   * by lfd_groupnorm_finalize_fold(which = 1 / 2), read by passes 2-3 / pass 3.  NULL: every work chunk folds on its own. */
  void* w1_folded;
  void* w2_folded;
  /* optional scratch, n * ceil(hw / 32) * LFD_HEAD_TOWER1_GROUP_HALFS halfs: ReLU(GN1(conv1)) of every pixel in fp16, as the MFMA
   * fragments pass 2 feeds its conv2 with.  Pass 2 writes it; when every level has it (and both folded filters) pass 3 /
   * lfd_head_forward_decode_f16 load it instead of recomputing neck + conv1: same bits, 45 instead of 101 MFMAs per 32 pixels. */
  void* tower1_out;
  /* optional: tower conv 1 / 2 in the kernel's K-permuted register layout (element e of lane (m, hk) of fragment (ct, k) =
   * W[32 ct + m][16 k + 8 (e >> 2) + 4 hk + (e & 3)], LFD_HEAD_FOLDED_HALFS - 4 * 64 * 8 halfs: no bias fragments), for the
   * passes that use the filter unscaled (conv1 in pass 1, conv2 in pass 2): plain 16-byte loads instead of a permute per
   * work chunk.  NULL: permuted from w1_packed / w2_packed on the fly. */
  const void* w1_perm;
  const void* w2_perm;
} lfd_head_level_ptrs_t;
#define LFD_HEAD_FOLDED_HALFS (4 * 9 * 64 * 8)
#define LFD_HEAD_TOWER1_GROUP_HALFS (8 * 64 * 8)

LFD_API size_t lfd_head_partial_floats(const lfd_head_desc_t* desc);
LFD_API int lfd_head_forward_f16(const lfd_head_desc_t* desc, int32_t pass,
                                 const lfd_head_level_ptrs_t* levels /*[num_levels], host array*/,
                                 const float* ab1 /*[L][n][128][2]*/, const float* ab2,
                                 float* partial, float* out_cls, float* out_reg, const void* zeros,
                                 lfd_stream_t stream);
/* The output pass (pass 3) for 64 < final_reg_rows + final_cls_rows <= 128: wf_packed / bf padded with zero rows to 32 * ft rows,
 * ft = ceil(rows / 32) = 3 or 4.  Passes 1 and 2 and both finalize calls are the entries above (they only validate the final
 * rows).  Same argument checks as lfd_head_forward_f16.  Runs in the wave-per-32-pixels kernel only: LFD_ERR_UNSUPPORTED, with
 * nothing launched, for up to 64 rows (use lfd_head_forward_f16), more than 128 rows, GroupNorm groups of fewer than 8 channels
 * and LFD_TUNE_HEAD2 = 0.  Class rows are written as 16-byte stores when final_reg_rows, final_cls_rows and cls_channels are
 * multiples of four and out_cls is 16-byte aligned, one by one otherwise: the same values either way. */
LFD_API int lfd_head_forward_wide_f16(const lfd_head_desc_t* desc, const lfd_head_level_ptrs_t* levels,
                                      const float* ab1, const float* ab2, float* out_cls, float* out_reg,
                                      const void* zeros, lfd_stream_t stream);
/* Pass 3 that also does the front half of lfd_detect_batched (lfd_head.py:164-185 + lfd.py:449-499 in one launch,
 * SURVEY 8b lfd_head_final_decode): sigma(cls) > score_thr -> decode -> append {box, score, label 0, point} to the
 * candidate arrays of `det_workspace`; lfd_detect_from_candidates finishes the step.  out_cls / out_reg may be NULL
 * (the fp32 [N,P,C'+4] logits then never reach HBM).  Supported: one foreground class with sigmoid scores, a merged
 * tower (final_reg_rows 4 + final_cls_rows 1), GroupNorm group size >= 8, det levels == head levels;
 * anything else returns LFD_ERR_UNSUPPORTED (use pass 3 + lfd_detect_batched). */
LFD_API int lfd_head_forward_decode_f16(const lfd_head_desc_t* desc, const lfd_head_level_ptrs_t* levels,
                                        const float* ab1, const float* ab2, float* out_cls, float* out_reg,
                                        const void* zeros, const lfd_detect_desc_t* det, const float* img_meta,
                                        void* det_workspace, size_t det_workspace_bytes, lfd_stream_t stream);
/* gamma / beta: host arrays of num_levels device pointers ([128] each). ab: [L][n][128][2]. */
LFD_API int lfd_groupnorm_finalize(const lfd_head_desc_t* desc, const float* partial,
                                   const float* const* gamma, const float* const* beta, float eps,
                                   float* ab, lfd_stream_t stream);
/* the same, and -- for every level whose w{which}_folded is not NULL -- the folded copy of tower conv `which` (1 | 2)
 * for each image (lfd_head_level_ptrs_t).  Same rounding as the in-kernel fold: fp16(fp32(w) * scale). */
LFD_API int lfd_groupnorm_finalize_fold(const lfd_head_desc_t* desc, const float* partial,
                                        const float* const* gamma, const float* const* beta, float eps, float* ab,
                                        const lfd_head_level_ptrs_t* levels, int32_t which, lfd_stream_t stream);

/* ---- training batch assembly (csrc/batch_assemble.hip) --------------------------------------------------------------------
 * The device tail of the reference loader for RandomBBoxCropRegionSampler / IdleRegionSampler
 * (lfd/data_pipeline/sampler/region_sampler.py:92-144,261-300, data_loader.py:68-124, augmentation_pipeline.py:14-36):
 * uint8 HWC source pixels -> cv2 INTER_LINEAR resize (8-bit fixed-point scalar path) -> crop (uint8 0 outside the resized
 * image) -> optional horizontal flip -> per-channel 256-entry fp32 table -> fp32 NCHW batch [n, c_out, h_out, w_out], 0.0f
 * outside each image's valid_w x valid_h extent (the batch padding).
 *
 * Each image reads only its source WINDOW: window pixel (x, y) is at src + src_offset + y * src_pitch + x * c_src, for
 * 0 <= x < win_w, 0 <= y < win_h, and holds source pixel (win_x0 + x, win_y0 + y).  The caller guarantees that every window
 * lies inside the memory behind `src`; the kernel clamps every table index into its window, so a wrong table gives wrong
 * pixels, never a read outside the window. */
typedef struct lfd_batch_desc {
  int64_t src_offset;       /* bytes from `src` to the window's first pixel */
  int32_t src_pitch;        /* bytes between window rows, >= win_w * c_src; win_h * src_pitch < 2^31 */
  int32_t win_x0, win_y0;   /* source coordinates of the window's first pixel */
  int32_t win_w, win_h;     /* window extent in pixels, >= 1 */
  int32_t valid_w, valid_h; /* the image's extent in the output (<= w_out, h_out); 0.0f beyond it */
  int32_t flip;             /* 1: output column x (< valid_w) reads crop column valid_w - 1 - x */
  int32_t reserved_;
} lfd_batch_desc_t;

/* coef: int32, image i at coef + 4 * i * (w_out + h_out): first w_out columns {sx0, sx1, a0, a1} (source columns of the two
 * taps and their 11-bit weights, indexed by crop column, i.e. before the flip), then h_out rows {r0, r1, b0, b1}.  A crop
 * column or row outside the resized image has zero weights (its value is uint8 0, as crop_from_image fills it).
 * Per channel c of the output: v = clamp((H(r0) * b0 + H(r1) * b1 + 2^21) >> 22, 0, 255) with
 * H(r) = S[r][sx0][map[c]] * a0 + S[r][sx1][map[c]] * a1, then out = lut[c * 256 + v].
 * lut: fp32 [c_out][256]; map: int32 [c_out], the source channel of each output channel (BGR2RGB = {2, 1, 0}, a gray
 * source tiled to 3 channels = {0, 0, 0}).
 * desc, map: 8-byte aligned; coef, lut, out: 16-byte aligned.  LFD_ERR_INVALID_ARGUMENT: a null or misaligned pointer,
 * c_src or c_out outside {1, 3}, n, h_out or w_out < 1; LFD_ERR_UNSUPPORTED: an output of 2^31 elements or more. */
LFD_API int lfd_batch_assemble_f32(const uint8_t* src, const lfd_batch_desc_t* desc /*[n], device*/,
                                   const int32_t* coef, const float* lut, const int32_t* map, int32_t n, int32_t c_src,
                                   int32_t c_out, int32_t h_out, int32_t w_out, float* out, lfd_stream_t stream);

/* ---- training batch planning (csrc/batch_plan.hip) ------------------------------------------------------------------------
 * Everything the host did per batch in front of lfd_batch_assemble_f32, for RandomBBoxCropRegionSampler over a dataset whose
 * decoded images and annotations are resident on the device (lfd_amd/data.py ResidentDataset): the sampler's draws, the scaled,
 * cropped and flipped boxes, the descriptors and the resize tables.  Two launches on `stream`: one workgroup per sample plans
 * it, then one workgroup scans the per-sample box counts and compacts the boxes.
 *
 * Draws ("the draw contract"): per sample two Philox4x32-10 blocks, key (seed & 0xffffffff, seed >> 32), counter
 * (slot i, batch, epoch, j), j = 0, 1 -> words r0..r7.  U(a, b) = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53; pick(r, n) = (r * n) >> 32.
 *   resize iff U(r0, r1) < resize_prob; scale = U(r2, r3) * (resize_hi - resize_lo) + resize_lo (double, no fma), else 1.0
 *   target box = pick(r4, G); crop_x = tx - (min(0, wr) + pick(r5, |wr| + 1)), wr = crop_size - tw; crop_y with r6;
 *   flip iff U(r7, r7) < flip_prob.  G = 0: target = {0, 0, res_w, res_h}.
 * The rest is the arithmetic of lfd_amd/data.py (RandomBBoxCropRegionSampler.__call__, flip_boxes, resized_size, plan_tables),
 * value for value; every output image is crop_size x crop_size.
 *
 * status (int32 [4], written by every call): [0] LFD_PLAN_* bits; [1] boxes dropped because a sample kept more than
 * max_boxes_per_image; [2] boxes dropped because the batch kept more than max_boxes (from the batch's tail); [3] samples
 * rendered as all zero without boxes (LFD_PLAN_EMPTY_RESIZE or LFD_PLAN_BAD_SAMPLE).  Nothing is written beyond a capacity. */
#define LFD_PLAN_EMPTY_RESIZE 1    /* rint(h * scale) or rint(w * scale) < 1 (cv2.resize asserts; resized_size raises) */
#define LFD_PLAN_IMAGE_OVERFLOW 2
#define LFD_PLAN_BATCH_OVERFLOW 4
#define LFD_PLAN_BAD_SAMPLE 8      /* a dataset index or a table entry out of range, or coordinates beyond 2^30 */
#define LFD_PLAN_MAX_BATCH 4096
typedef struct lfd_plan_desc {
  uint64_t seed;
  double resize_lo, resize_hi, resize_prob, flip_prob;
  int64_t arena_bytes;          /* bytes behind the image arena: an image that does not fit is LFD_PLAN_BAD_SAMPLE */
  uint32_t epoch, batch;
  int32_t n;                    /* samples in the batch, 1 .. LFD_PLAN_MAX_BATCH */
  int32_t num_images;           /* M: rows of img_offset / img_h / img_w */
  int32_t total_boxes;          /* rows of box / label */
  int32_t crop_size, c_src;     /* c_src: channels of every stored image (1 | 3) */
  int32_t max_boxes_per_image, max_boxes;
  int32_t reserved_;
} lfd_plan_desc_t;
typedef struct lfd_plan_bufs {
  /* the dataset (read only) */
  const int64_t* img_offset;    /* [M] bytes from the arena's start to image m, HWC uint8 with c_src channels */
  const int32_t* img_h;         /* [M] */
  const int32_t* img_w;         /* [M] */
  const double* box;            /* [total_boxes, 4] x, y, w, h */
  const int64_t* label;         /* [total_boxes] */
  const int32_t* box_offset;    /* [M + 1] image m owns boxes box_offset[m] .. box_offset[m + 1] */
  const int32_t* indices;       /* [n] dataset index of every slot of this batch */
  /* for lfd_batch_assemble_f32 (h_out = w_out = crop_size) */
  lfd_batch_desc_t* desc;       /* [n], 8-byte aligned */
  int32_t* coef;                /* [n, 2 * crop_size, 4], 16-byte aligned */
  /* staging, per sample */
  float* stage_box;             /* [n, max_boxes_per_image, 4], 16-byte aligned */
  int64_t* stage_label;         /* [n, max_boxes_per_image] */
  int32_t* stage_count;         /* [n, 4]: kept (clipped), dropped, LFD_PLAN_* bits of the sample, reserved */
  /* the batch's annotations, GraphedTrainStep's layout */
  float* boxes;                 /* [max_boxes, 4] x, y, w, h, 16-byte aligned */
  int64_t* labels;              /* [max_boxes] */
  int32_t* offsets;             /* [n + 1] */
  int32_t* status;              /* [4] */
} lfd_plan_bufs_t;
/* LFD_ERR_INVALID_ARGUMENT: a null or misaligned pointer, n < 1, crop_size < 1, c_src outside {1, 3}, a capacity < 1,
 * resize_lo / resize_hi not finite; LFD_ERR_UNSUPPORTED: n > LFD_PLAN_MAX_BATCH or an assembled output of 2^31
 * elements or more. */
LFD_API int lfd_plan_bbox_crop_batch(const lfd_plan_desc_t* d, const lfd_plan_bufs_t* b, lfd_stream_t stream);

/* ---- detection evaluation: COCO-style bbox AP (csrc/evaluate.hip) -----------------------------------------------------------
 * The device side of lfd_amd/evaluation.py (the reference's COCOEvaluator, lfd/evaluation/coco_evaluator.py:13-82, which hands
 * its detections to pycocotools).  The definition implemented is written out in DESIGN.md ("Evaluation"); it restates
 * COCOeval (iouType 'bbox', useCats 1) from knowledge of pycocotools 2.0.x and is NOT verified against pycocotools itself.
 * All IoU / precision / recall arithmetic is float64, evaluated operation for operation as that text states it.
 *
 * Images are addressed by their ordinal in ascending image id, categories by their index in ascending category id; a
 * (image, category) pair is p = image * num_categories + category.  Boxes are {x, y, w, h}.
 * Everything behind lfd_eval_bufs_t is device memory owned by the caller.  The entry points enqueue on `stream` and never
 * synchronise; what only the device knows (the number of stored detections, capacity overflows) is kept in `state`:
 *   state[0] detections stored; state[1] error bits (LFD_EVAL_ERR_*), sticky until the caller clears them;
 *   state[2] detections that take part in the last lfd_eval_match (known category, evaluated image); state[3] active pairs.
 * The caller zeroes state and img_mask to start (or restart) an accumulation. */
#define LFD_EVAL_MAX_MAXDETS 8
#define LFD_EVAL_MAX_RECTHRS 256
#define LFD_EVAL_ERR_CAPACITY 1   /* an append did not fit det_capacity: nothing of that append was stored */
#define LFD_EVAL_ERR_IMAGE 2      /* an image ordinal outside [0, num_images) */
#define LFD_EVAL_ERR_LABEL 4      /* a label without a category (lfd_eval_append_dets_f32): the detection was dropped */
typedef struct lfd_eval_desc {
  int32_t num_images, num_categories, num_gt, det_capacity;
  int32_t num_iou_thrs, num_area_rngs;   /* T, A; T * A <= 64 */
  int32_t num_rec_thrs, num_max_dets;    /* R <= LFD_EVAL_MAX_RECTHRS, M <= LFD_EVAL_MAX_MAXDETS */
  int32_t max_dets[LFD_EVAL_MAX_MAXDETS]; /* ascending; detections of a pair beyond max_dets[M-1] are not matched */
} lfd_eval_desc_t;
typedef struct lfd_eval_bufs {
  /* the detection store, in insertion order */
  double* det_box;            /* [det_capacity, 4] */
  double* det_score;          /* [det_capacity] */
  int32_t* det_img;           /* [det_capacity] image ordinal */
  int32_t* det_cat;           /* [det_capacity] category index, -1: no category (never evaluated) */
  int32_t* state;             /* [4], see above */
  int32_t* img_mask;          /* [num_images] 1: the image is evaluated */
  /* ground truth, sorted by pair (stable: annotation order inside a pair) */
  const double* gt_box;       /* [num_gt, 4] */
  const double* gt_area;      /* [num_gt] */
  const int32_t* gt_crowd;    /* [num_gt] */
  const int32_t* gt_pair_start; /* [num_images * num_categories + 1] first ground truth of each pair */
  /* parameters, computed by the caller (numpy linspace) and only read here */
  const double* iou_thrs;     /* [T] */
  const double* area_rng;     /* [A, 2] {lo, hi} */
  const double* rec_thrs;     /* [R] */
  /* lfd_eval_match -> lfd_eval_accumulate: one entry per participating detection, pair-major, rank order inside a pair */
  int32_t* order;             /* [det_capacity] index into the store */
  uint64_t* sort_key;         /* [det_capacity] descending-score key */
  int32_t* sorted_cat;        /* [det_capacity] */
  int32_t* sorted_rank;       /* [det_capacity] rank inside the pair (score descending, ties in insertion order) */
  uint64_t* match_bits;       /* [det_capacity] bit t * A + a: matched at threshold t in area range a */
  uint64_t* ignore_bits;      /* [det_capacity] same layout: ignored */
  int32_t* npig;              /* [num_categories, A] non-ignored ground truth of the evaluated images */
  int32_t* cat_start;         /* [num_categories + 1] first entry of each category once sorted by category */
  /* results */
  double* precision;          /* [T, R, K, A, M], -1: no non-ignored ground truth */
  double* recall;             /* [T, K, A, M] */
} lfd_eval_bufs_t;

/* Append the kept boxes of a detection step (lfd_detect_batched outputs: dets [n, cap, 5] = {x1, y1, x2, y2, score},
 * labels [n, cap], counts [n, 4] with the number kept in counts[i][1], read on the device) as {x1, y1, x2 - x1 + 1,
 * y2 - y1 + 1} (fp32 arithmetic, then widened).  label_map [num_labels]: category index of each label, -1: none.
 * img_ord [n] (device): image ordinal of each batch entry.  An image is marked for evaluation when it contributed a box,
 * or always with mark_all != 0. */
LFD_API int lfd_eval_append_dets_f32(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, const float* dets,
                                     const int32_t* labels, const int32_t* counts, int32_t n, int32_t cap,
                                     const int32_t* label_map, int32_t num_labels, const int32_t* img_ord,
                                     int32_t mark_all, lfd_stream_t stream);
/* Append m rows {image ordinal, category index, score, x, y, w, h} (float64, device) and mark their images; `mark`
 * [num_mark] (device, may be NULL with num_mark 0) lists further image ordinals to mark. */
LFD_API int lfd_eval_append_rows_f64(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, const double* rows, int64_t m,
                                     const int32_t* mark, int32_t num_mark, lfd_stream_t stream);
/* Stage 1: groups the stored detections by pair, ranks each pair's detections by score (stable) and runs the greedy
 * matching of every pair that has a detection or a ground-truth box, for all T thresholds and A area ranges.  One
 * workgroup per active pair (a persistent grid walks the compacted pair list, never the dense images x categories grid);
 * ground truth is processed in tiles of 64, any number per pair. */
LFD_API size_t lfd_eval_match_workspace_bytes(const lfd_eval_desc_t* desc);
LFD_API int lfd_eval_match(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, void* workspace, size_t workspace_bytes,
                           lfd_stream_t stream);
/* Stage 2: stable sort by (category, score descending) of what stage 1 left, then per (category, area range, max_dets
 * entry, threshold) the running true / false positive counts, the precision envelope and its samples at the recall points. */
LFD_API size_t lfd_eval_accumulate_workspace_bytes(const lfd_eval_desc_t* desc);
LFD_API int lfd_eval_accumulate(const lfd_eval_desc_t* desc, const lfd_eval_bufs_t* bufs, void* workspace,
                                size_t workspace_bytes, lfd_stream_t stream);

/* ---- detection evaluation: the TT100K protocol, accuracy / recall (csrc/evaluate_tt100k.hip) -------------------------------
 * The device side of lfd_amd/evaluation.py TT100KEvaluator: eval_annos of the reference's TT100K_train/official_eval.py
 * (called from TT100K_train/evaluation.py:70-79), restated in DESIGN.md 9b.  Per evaluated image one global greedy matching
 * in IoU-descending order (ties: ground-truth index, then detection index; strict IoU > iou), computed once per
 * (iou, minscore) and read by every size band.  All arithmetic is float64, evaluated as the definition writes it.
 *
 * The detection store, `state` and `img_mask` work as in lfd_eval_bufs_t (same LFD_EVAL_ERR_* bits); boxes are
 * {xmin, ymin, xmax, ymax} and scores are scaled to 0..100.  Every image named by an append is evaluated, with or without
 * detections.  state[2]: detections grouped by the last lfd_eval_tt100k_match.  Cells are indexed [iou, minscore, size range]. */
#define LFD_TT100K_DET_EXCLUDED 0   /* outside `types`, below minscore, outside the size band, or matched to such a ground truth */
#define LFD_TT100K_DET_RIGHT 1
#define LFD_TT100K_DET_WRONG 2      /* matched to a ground truth of another category (check_type) */
#define LFD_TT100K_DET_UNMATCHED 3
#define LFD_TT100K_GT_EXCLUDED 0
#define LFD_TT100K_GT_MISSED 1
#define LFD_TT100K_GT_MATCHED 2
typedef struct lfd_eval_tt100k_desc {
  int32_t num_images, num_categories, num_gt, det_capacity;
  int32_t num_ious, num_minscores, num_size_ranges;   /* T, M, S >= 1; T * M <= 4096 */
  int32_t check_type, match_same;
} lfd_eval_tt100k_desc_t;
typedef struct lfd_eval_tt100k_bufs {
  /* the detection store, in insertion order */
  double* det_box;             /* [det_capacity, 4] {xmin, ymin, xmax, ymax} */
  double* det_score;           /* [det_capacity] 0..100 */
  int32_t* det_img;            /* [det_capacity] image ordinal */
  int32_t* det_cat;            /* [det_capacity] category index, -1: none */
  int32_t* state;              /* [4] */
  int32_t* img_mask;           /* [num_images] 1: the image is evaluated */
  /* ground truth, sorted by image (stable: annotation order inside an image) */
  const double* gt_box;        /* [num_gt, 4] {xmin, ymin, xmax, ymax} */
  const int32_t* gt_cat;       /* [num_gt] category index */
  const int32_t* gt_start;     /* [num_images + 1] */
  const int32_t* cat_in_types; /* [num_categories] 1: the category takes part (all 1: no category filter) */
  const double* ious;          /* [T] */
  const double* minscores;     /* [M] */
  const double* size_ranges;   /* [S, 2] {minboxsize, maxboxsize} */
  /* results of lfd_eval_tt100k_match; "grouped" positions are image-major, insertion order inside an image */
  int32_t* det_start;          /* [num_images + 1] first grouped position of each image */
  int32_t* det_index;          /* [det_capacity] grouped position -> index into the store */
  int32_t* det_match;          /* [T * M, det_capacity] per grouped position: matched ground truth (index inside its image), -1
                                  unmatched, -2 taken out before the matching */
  int32_t* gt_match;           /* [T * M, num_gt] matched detection (index inside its image), -1, -2 */
  uint64_t* totals;            /* [T, M, S, 3] {right, counted detections, counted ground truth} */
  uint64_t* per_category;      /* [T, M, S, num_categories, 3] the same by category, or NULL */
  uint8_t* det_code;           /* [T, M, S, det_capacity] LFD_TT100K_DET_* per grouped position, or NULL */
  uint8_t* gt_code;            /* [T, M, S, num_gt] LFD_TT100K_GT_*, or NULL */
} lfd_eval_tt100k_bufs_t;

/* Append the kept boxes of a detection step (as lfd_eval_append_dets_f32 reads them) the way the reference's
 * TT100K_train/evaluation.py:42-55 builds its results: w = x2 - x1 + 1 and h in fp32, then xmax = (double)w + (double)x1,
 * ymax likewise, score = (double)score * 100.  Every batch entry's image is marked for evaluation. */
LFD_API int lfd_eval_tt100k_append_dets_f32(const lfd_eval_tt100k_desc_t* desc, const lfd_eval_tt100k_bufs_t* bufs,
                                            const float* dets, const int32_t* labels, const int32_t* counts, int32_t n,
                                            int32_t cap, const int32_t* label_map, int32_t num_labels, const int32_t* img_ord,
                                            lfd_stream_t stream);
/* Append m rows {image ordinal, category index, score, x, y, w, h} (float64, device): score * 100, xmax = w + x, ymax = h + y;
 * `mark` [num_mark] (device, may be NULL with num_mark 0) lists image ordinals to evaluate whether or not they have a row. */
LFD_API int lfd_eval_tt100k_append_rows_f64(const lfd_eval_tt100k_desc_t* desc, const lfd_eval_tt100k_bufs_t* bufs,
                                            const double* rows, int64_t m, const int32_t* mark, int32_t num_mark,
                                            lfd_stream_t stream);
/* Groups the store by image in insertion order, runs the matching of every evaluated image for all T * M (iou, minscore)
 * pairs (one workgroup each; IoU tile in LDS when it fits, recomputed round by round when not: any number of boxes per
 * image), applies the S size bands and sums the counts (integer atomics: the result does not depend on the schedule). */
LFD_API size_t lfd_eval_tt100k_workspace_bytes(const lfd_eval_tt100k_desc_t* desc);
LFD_API int lfd_eval_tt100k_match(const lfd_eval_tt100k_desc_t* desc, const lfd_eval_tt100k_bufs_t* bufs, void* workspace,
                                  size_t workspace_bytes, lfd_stream_t stream);

/* ---- detection evaluation: the WIDERFACE protocol, easy / medium / hard AP (csrc/evaluate_widerface.hip) --------------------
 * The device side of lfd_amd/evaluation.py WIDERFACEEvaluator; the definition is DESIGN.md 9c, a restatement of the
 * dataset's eval_tools from knowledge of them that is NOT verified against those tools.  Per image the detections are ranked
 * by score (stable), every detection takes the first ground truth of maximal IoU (+1 convention), and per difficulty a
 * sequential walk in rank order gives the running proposal and recall counts, which are sampled at num_thresholds thresholds
 * of the normalised score and summed over the images into `curve`.  All arithmetic is float64, evaluated as the definition
 * writes it; the results are integers.
 *
 * The detection store and `state` work as in lfd_eval_bufs_t (same LFD_EVAL_ERR_* bits; there is one class and no
 * img_mask); boxes are {x, y, w, h}.  A stored row with det_img = -1 (a label the caller filters out) takes part in nothing.
 * state[2]: detections grouped by the last lfd_eval_wf_match.  Difficulties are indexed 0 easy, 1 medium, 2 hard. */
typedef struct lfd_eval_wf_desc {
  int32_t num_images, num_gt, det_capacity;
  int32_t num_thresholds;      /* T <= 1024 */
  int32_t as_written;          /* lfd_eval_wf_append_dets_f32 quantises as the reference's text files do and adds their dummy row */
  int32_t label_index;         /* lfd_eval_wf_append_dets_f32 keeps this label only; < 0: every label */
  double iou_thresh;
} lfd_eval_wf_desc_t;
typedef struct lfd_eval_wf_bufs {
  /* the detection store, in insertion order */
  double* det_box;             /* [det_capacity, 4] {x, y, w, h} */
  double* det_score;           /* [det_capacity] */
  int32_t* det_img;            /* [det_capacity] image ordinal, -1: dropped */
  int32_t* state;              /* [4] */
  /* ground truth, sorted by image (annotation order inside an image) */
  const double* gt_box;        /* [num_gt, 4] {x, y, w, h} */
  const int32_t* gt_start;     /* [num_images + 1] */
  const uint8_t* gt_kept;      /* [num_gt] bit d: the box is in difficulty d's keep list */
  const int32_t* keep_len;     /* [num_images, 3] length of each keep list */
  const double* thr;           /* [T] score thresholds, descending */
  /* results of lfd_eval_wf_match; "grouped" positions are image-major, rank order inside an image */
  int32_t* det_start;          /* [num_images + 1] first grouped position of each image */
  int32_t* det_index;          /* [det_capacity] grouped position -> index into the store */
  int32_t* det_gt;             /* [det_capacity] first ground truth of maximal IoU (index inside its image) */
  uint8_t* det_over;           /* [det_capacity] 1: that IoU >= iou_thresh */
  int32_t* det_prop;           /* [3, det_capacity] running proposal count inside the image, per difficulty */
  int32_t* det_rec;            /* [3, det_capacity] running recalled-face count */
  uint8_t* det_flags;          /* [det_capacity] bit 0: det_over, bit 1 + d: proposal of difficulty d; or NULL */
  uint64_t* curve;             /* [3, T, 2] {proposals, recalled faces} at each threshold, summed over the images */
  uint64_t* faces;             /* [3] keep-list lengths summed over every annotated image */
  double* minmax;              /* [2] minimum and maximum stored score, or NULL */
} lfd_eval_wf_bufs_t;
/* grouped positions of images without ground truth are not ranked: their det_index .. det_flags entries are not written */

/* Append the kept boxes of a detection step (as lfd_eval_append_dets_f32 reads them): w = x2 - x1 + 1 and h in fp32, then
 * widened.  With desc->as_written every batch entry first gets the row {0, 0, 0, 0, 0.001} and every box is stored as
 * {floor x, floor y, ceil w, ceil h} with the score min(s, 1) rounded to three decimals (half to even, decided exactly). */
LFD_API int lfd_eval_wf_append_dets_f32(const lfd_eval_wf_desc_t* desc, const lfd_eval_wf_bufs_t* bufs, const float* dets,
                                        const int32_t* labels, const int32_t* counts, int32_t n, int32_t cap,
                                        const int32_t* img_ord, lfd_stream_t stream);
/* Append m rows {image ordinal, score, x, y, w, h} (float64, device) as they are. */
LFD_API int lfd_eval_wf_append_rows_f64(const lfd_eval_wf_desc_t* desc, const lfd_eval_wf_bufs_t* bufs, const double* rows,
                                        int64_t m, lfd_stream_t stream);
/* Score range, grouping by image, and one persistent grid over the images: rank, IoU argmax over 64-wide ground-truth
 * tiles, the walk per difficulty, the threshold sweep (integer atomics: the result does not depend on the schedule). */
LFD_API size_t lfd_eval_wf_workspace_bytes(const lfd_eval_wf_desc_t* desc);
LFD_API int lfd_eval_wf_match(const lfd_eval_wf_desc_t* desc, const lfd_eval_wf_bufs_t* bufs, void* workspace,
                              size_t workspace_bytes, lfd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Eval-mode BatchNorm inside a training iteration (csrc/train_bn_eval.hip): fine-tuning with LFDResNet(frozen_stages=k,
 * norm_eval=True) (lfd/model/backbone/lfd_resnet.py:476-509).  An eval-mode norm normalises with its running statistics
 * and updates nothing.
 */
/* running_mean / running_var / eps of every eval-mode norm -> its stats row float32[2 * channels] = (mean, 1 / sqrt(var + eps)),
 * the layout lfd_bn_train_apply_f16 reads: one launch over a job table in device memory.  max_channels >= every job's channels. */
typedef struct lfd_bn_eval_job {
  const float* running_mean;
  const float* running_var;
  float* stats;
  int32_t channels;
  float eps;
} lfd_bn_eval_job_t;
LFD_API int lfd_bn_eval_stats_f32(const lfd_bn_eval_job_t* jobs_device, int32_t njobs, int32_t max_channels, lfd_stream_t stream);
/* Frozen Conv2d(bias=False) -> eval-mode BatchNorm2d units as ONE conv with bias: w_out = w * gamma * rstd (per output row),
 * bias_out = beta - mean * gamma * rstd, both fp32, from the stats rows above.  One launch over a job table in device memory,
 * first_elem ascending from 0, total_elems = sum of cout * row_elems (row_elems = cin * ks * ks). */
typedef struct lfd_bn_fold_job {
  const float* w;
  const float* gamma;
  const float* beta;
  const float* stats;
  float* w_out;
  float* bias_out;
  int32_t cout, row_elems, first_elem, reserved_;
} lfd_bn_fold_job_t;
LFD_API int lfd_conv_bn_eval_fold_f32(const lfd_bn_fold_job_t* jobs_device, int32_t njobs, int32_t total_elems, lfd_stream_t stream);
/* Backward of z = relu?(gamma * (y - mean) * rstd + beta (+ residual)) with CONSTANT (mean, rstd) in `stats`, in ONE pass over
 * (dz, y):  g = dz * mask,  dy = gamma * rstd * g,  dgamma (+)= sum(g * xhat) * inv_scale,  dbeta (+)= sum(g) * inv_scale.
 * Arguments as lfd_bn_train_bwd_f16: z nullable (with relu != 0 and z == NULL the mask is recomputed from y, beta required),
 * g_out nullable (the gradient of the residual branch), dgamma / dbeta nullable together with the final launch, `workspace`
 * lfd_train_workspace_bytes().  fp32 per-block partial sums + a fixed-order fp64 final: deterministic. */
LFD_API int lfd_bn_eval_bwd_f16(const void* dz, const void* y, const void* z, int32_t relu, int64_t pixels, int32_t channels,
                        const float* stats, const float* gamma, const float* beta, float inv_scale, int32_t accumulate,
                        void* workspace, size_t workspace_bytes, float* dgamma, float* dbeta, void* dy, void* g_out,
                        lfd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LFD_HIP_H_ */
