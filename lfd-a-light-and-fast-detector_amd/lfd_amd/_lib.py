"""ctypes binding of liblfd_hip.so (C ABI: include/lfd_hip.h).

This is the ONLY compute backend of the package.  There is no PyTorch / CPU fallback: if the
library is missing or a call fails, a RuntimeError is raised (the reference raises the same
way through AT_ERROR / TORCH_CHECK -> RuntimeError, nms_ext.cpp:22-24).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LFD_HIP_LIB: load another build of the same ABI (A/B timing of kernel variants inside one GPU session)
LIB_PATH = os.environ.get('LFD_HIP_LIB') or os.path.join(_HERE, 'liblfd_hip.so')
MAX_LEVELS = 8
F32, F16 = 0, 1

_lib = None


class DetectDesc(C.Structure):
    """lfd_detect_desc_t"""
    _fields_ = [('num_levels', C.c_int32),
                ('level_h', C.c_int32 * MAX_LEVELS), ('level_w', C.c_int32 * MAX_LEVELS),
                ('level_stride', C.c_int32 * MAX_LEVELS),
                ('level_range_lo', C.c_float * MAX_LEVELS), ('level_range_hi', C.c_float * MAX_LEVELS),
                ('num_classes', C.c_int32), ('num_cls_channels', C.c_int32),
                ('score_mode', C.c_int32), ('decode_mode', C.c_int32),
                ('class_agnostic', C.c_int32), ('max_candidates', C.c_int32),
                ('score_thr', C.c_float), ('iou_thr', C.c_float)]


class DetectExt(C.Structure):
    """lfd_detect_ext_t"""
    _fields_ = [('pre_nms_limit', C.c_int32), ('post_nms_limit', C.c_int32)]


class ConvDesc(C.Structure):
    """lfd_conv_desc_t"""
    _fields_ = [('n', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('cin', C.c_int32), ('cout', C.c_int32),
                ('ks', C.c_int32), ('stride', C.c_int32), ('relu', C.c_int32), ('tail_cout', C.c_int32),
                ('tail_relu', C.c_int32)]


class HeadOutSeg(C.Structure):
    """lfd_head_out_seg_t"""
    _fields_ = [('out', C.c_void_p), ('grad', C.c_void_p), ('dbias', C.c_void_p), ('scale', C.c_void_p),
                ('dscale', C.c_void_p), ('channels', C.c_int32), ('row0', C.c_int32)]


class HeadOutLevel(C.Structure):
    """lfd_head_out_level_t"""
    _fields_ = [('hw', C.c_int32), ('nsegs', C.c_int32), ('point0', C.c_int64), ('segs', HeadOutSeg * 2)]


class FcosOutLevel(C.Structure):
    """lfd_fcos_out_level_t"""
    _fields_ = [('raw_cls', C.c_void_p), ('raw_reg', C.c_void_p), ('scale', C.c_void_p), ('dscale', C.c_void_p),
                ('dy_cls', C.c_void_p), ('dy_reg', C.c_void_p), ('hw', C.c_int32), ('reserved', C.c_int32), ('point0', C.c_int64)]


class LfdHeadOutSeg(C.Structure):
    """lfd_lfdhead_out_seg_t"""
    _fields_ = [('dbias', C.c_void_p), ('row0', C.c_int32), ('channels', C.c_int32), ('kind', C.c_int32), ('reserved', C.c_int32)]


class LfdHeadOutConv(C.Structure):
    """lfd_lfdhead_out_conv_t"""
    _fields_ = [('raw', C.c_void_p), ('dy', C.c_void_p), ('nsegs', C.c_int32), ('reserved', C.c_int32), ('segs', LfdHeadOutSeg * 2)]


class LfdHeadOutLevel(C.Structure):
    """lfd_lfdhead_out_level_t"""
    _fields_ = [('scale', C.c_void_p), ('dscale', C.c_void_p), ('hw', C.c_int32), ('nconvs', C.c_int32), ('point0', C.c_int64),
                ('convs', LfdHeadOutConv * 2)]


class BnBwdLevel(C.Structure):
    """lfd_bn_bwd_level_t"""
    _fields_ = [('y', C.c_void_p), ('dy', C.c_void_p), ('stats', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p),
                ('dgamma', C.c_void_p), ('dbeta', C.c_void_p), ('hw', C.c_int64), ('point0', C.c_int64), ('channels', C.c_int32),
                ('reserved_', C.c_int32)]


class BnFwdLevel(C.Structure):
    """lfd_bn_fwd_level_t"""
    _fields_ = [('y', C.c_void_p), ('rows', C.c_void_p), ('running_mean', C.c_void_p), ('running_var', C.c_void_p),
                ('stats', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p), ('hw', C.c_int64), ('point0', C.c_int64),
                ('channels', C.c_int32), ('nrows', C.c_int32), ('eps', C.c_float), ('momentum', C.c_float)]


class HeadDesc(C.Structure):
    """lfd_head_desc_t"""
    _fields_ = [('n', C.c_int32), ('num_levels', C.c_int32), ('level_hw', C.c_int32 * MAX_LEVELS),
                ('level_cin', C.c_int32 * MAX_LEVELS), ('level_point_offset', C.c_int32 * MAX_LEVELS),
                ('head_channels', C.c_int32), ('num_groups', C.c_int32), ('total_points', C.c_int32),
                ('cls_channels', C.c_int32), ('final_reg_rows', C.c_int32), ('final_cls_rows', C.c_int32)]


class HeadLevelPtrs(C.Structure):
    """lfd_head_level_ptrs_t"""
    _fields_ = [('x', C.c_void_p), ('wn_packed', C.c_void_p), ('bn', C.c_void_p), ('w1_packed', C.c_void_p),
                ('w2_packed', C.c_void_p), ('wf_packed', C.c_void_p), ('bf', C.c_void_p), ('scale', C.c_void_p),
                ('w1_folded', C.c_void_p), ('w2_folded', C.c_void_p), ('tower1_out', C.c_void_p),
                ('w1_perm', C.c_void_p), ('w2_perm', C.c_void_p)]


class P32ConvDesc(C.Structure):
    """lfd_p32_conv_desc_t"""
    _fields_ = [('n', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('cin', C.c_int32), ('cout', C.c_int32),
                ('ks', C.c_int32), ('stride', C.c_int32), ('relu', C.c_int32), ('in_format', C.c_int32),
                ('out_pixel_stride', C.c_int32), ('out_image_stride', C.c_int64)]


class PlConvDesc(C.Structure):
    """lfd_pl_conv_desc_t"""
    _fields_ = [('n', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('cin', C.c_int32), ('cout', C.c_int32),
                ('ks', C.c_int32), ('stride', C.c_int32), ('relu', C.c_int32), ('tail_cout', C.c_int32),
                ('tail_relu', C.c_int32), ('out_mode', C.c_int32), ('f_c0', C.c_int32), ('f_c1', C.c_int32),
                ('gn_in_eps', C.c_float), ('in_plane_halfs', C.c_int64), ('out_plane_halfs', C.c_int64),
                ('res_plane_halfs', C.c_int64), ('ds_plane_halfs', C.c_int64), ('f_image_stride0', C.c_int64),
                ('f_image_stride1', C.c_int64)]


class PlLevel(C.Structure):
    """lfd_pl_level_t"""
    _fields_ = [(k, C.c_void_p) for k in ('in_', 'out', 'w_packed', 'bias', 'tail_w_packed', 'tail_bias', 'gn_sums', 'gn_in_sums',
                                          'gn_in_gamma', 'gn_in_beta', 'f_out0', 'f_out1', 'scale1')] + \
               [('h', C.c_int32), ('w', C.c_int32), ('in_plane_halfs', C.c_int64), ('out_plane_halfs', C.c_int64)]


class PlHeadDesc(C.Structure):
    """lfd_pl_head_desc_t"""
    _fields_ = [('mode', C.c_int32), ('n', C.c_int32), ('cin', C.c_int32), ('relu0', C.c_int32), ('f_c0', C.c_int32), ('f_c1', C.c_int32),
                ('gn_in_eps', C.c_float), ('pad_', C.c_int32), ('f_image_stride0', C.c_int64), ('f_image_stride1', C.c_int64)]


class PlHeadLevel(C.Structure):
    """lfd_pl_head_level_t"""
    _fields_ = [(k, C.c_void_p) for k in ('in_', 'out', 'w0', 'b0', 'w1', 'b1', 'gn_sums', 'gn_in_sums', 'gn_in_gamma', 'gn_in_beta',
                                          'f_out0', 'f_out1', 'scale1')] + \
               [('in_plane_halfs', C.c_int64), ('pixels', C.c_int32), ('pad_', C.c_int32)]


PL_GN_REPLICAS = 8                      # LFD_PL_GN_REPLICAS
ABI_VERSION = 3                         # LFD_HIP_ABI_VERSION
HEAD_FOLDED_HALFS = 4 * 9 * 64 * 8      # LFD_HEAD_FOLDED_HALFS
HEAD_TOWER1_GROUP_HALFS = 8 * 64 * 8    # LFD_HEAD_TOWER1_GROUP_HALFS


class AssignDesc(C.Structure):
    """lfd_assign_desc_t"""
    _fields_ = [('n', C.c_int32), ('num_levels', C.c_int32),
                ('level_h', C.c_int32 * MAX_LEVELS), ('level_w', C.c_int32 * MAX_LEVELS), ('stride', C.c_int32 * MAX_LEVELS),
                ('reg_lo', C.c_int32 * MAX_LEVELS), ('reg_hi', C.c_int32 * MAX_LEVELS),
                ('gray_lo', C.c_int32 * MAX_LEVELS), ('gray_hi', C.c_int32 * MAX_LEVELS),
                ('total_points', C.c_int32), ('num_classes', C.c_int32),
                ('assign_mode', C.c_int32), ('independent', C.c_int32)]


class LossDesc(C.Structure):
    """lfd_loss_desc_t"""
    _fields_ = [('n', C.c_int32), ('num_levels', C.c_int32),
                ('level_h', C.c_int32 * MAX_LEVELS), ('level_w', C.c_int32 * MAX_LEVELS), ('stride', C.c_int32 * MAX_LEVELS),
                ('range_max', C.c_float * MAX_LEVELS),
                ('total_points', C.c_int32), ('num_classes', C.c_int32),
                ('cls_loss', C.c_int32), ('decode_mode', C.c_int32),
                ('gamma', C.c_float), ('alpha', C.c_float), ('iou_eps', C.c_float),
                ('cls_loss_weight', C.c_float), ('reg_loss_weight', C.c_float),
                ('cls_weighted', C.c_int32), ('reg_weighted', C.c_int32)]


class LossDescEx(C.Structure):
    """lfd_loss_ex_desc_t"""
    _fields_ = [('n', C.c_int32), ('num_levels', C.c_int32),
                ('level_h', C.c_int32 * MAX_LEVELS), ('level_w', C.c_int32 * MAX_LEVELS), ('stride', C.c_int32 * MAX_LEVELS),
                ('range_max', C.c_float * MAX_LEVELS),
                ('total_points', C.c_int32), ('num_classes', C.c_int32),
                ('cls_loss', C.c_int32), ('reg_loss', C.c_int32), ('decode_mode', C.c_int32),
                ('gamma', C.c_float), ('alpha', C.c_float), ('qfl_beta', C.c_float), ('smooth_l1_beta', C.c_float),
                ('box_eps', C.c_float),
                ('cls_loss_weight', C.c_float), ('reg_loss_weight', C.c_float),
                ('cls_weighted', C.c_int32), ('reg_weighted', C.c_int32)]


class AssignFcosDesc(C.Structure):
    """lfd_assign_fcos_desc_t"""
    _fields_ = [('n', C.c_int32), ('num_levels', C.c_int32),
                ('level_h', C.c_int32 * MAX_LEVELS), ('level_w', C.c_int32 * MAX_LEVELS), ('stride', C.c_int32 * MAX_LEVELS),
                ('range_lo', C.c_float * MAX_LEVELS), ('range_hi', C.c_float * MAX_LEVELS),
                ('total_points', C.c_int32), ('num_classes', C.c_int32),
                ('multi_label', C.c_int32), ('reserved_', C.c_int32)]


class FcosLossDesc(C.Structure):
    """lfd_fcos_loss_desc_t"""
    _fields_ = [('n', C.c_int32), ('num_levels', C.c_int32),
                ('level_h', C.c_int32 * MAX_LEVELS), ('level_w', C.c_int32 * MAX_LEVELS), ('stride', C.c_int32 * MAX_LEVELS),
                ('total_points', C.c_int32), ('num_classes', C.c_int32),
                ('multi_label', C.c_int32), ('box_loss', C.c_int32),
                ('gamma', C.c_float), ('alpha', C.c_float), ('box_eps', C.c_float),
                ('cls_loss_weight', C.c_float), ('reg_loss_weight', C.c_float), ('ctr_loss_weight', C.c_float)]


class PackJob(C.Structure):
    """lfd_pack_job_t"""
    _fields_ = [('w', C.c_void_p), ('out', C.c_void_p), ('cout', C.c_int32), ('cin', C.c_int32), ('ks', C.c_int32),
                ('mode', C.c_int32), ('rows_valid', C.c_int32), ('first_vec', C.c_int32)]


class BnEvalJob(C.Structure):
    """lfd_bn_eval_job_t"""
    _fields_ = [('running_mean', C.c_void_p), ('running_var', C.c_void_p), ('stats', C.c_void_p), ('channels', C.c_int32),
                ('eps', C.c_float)]


class BnFoldJob(C.Structure):
    """lfd_bn_fold_job_t"""
    _fields_ = [('w', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p), ('stats', C.c_void_p), ('w_out', C.c_void_p),
                ('bias_out', C.c_void_p), ('cout', C.c_int32), ('row_elems', C.c_int32), ('first_elem', C.c_int32),
                ('reserved_', C.c_int32)]


class WgradJob(C.Structure):
    """lfd_wgrad_job_t"""
    _fields_ = [('partials', C.c_void_p), ('dw', C.c_void_p), ('nwg', C.c_int32), ('nblk', C.c_int32), ('cin', C.c_int32),
                ('cout', C.c_int32), ('taps', C.c_int32), ('co_lo', C.c_int32), ('co_hi', C.c_int32),
                ('first_block', C.c_int32), ('next', C.c_int32), ('accumulate', C.c_int32), ('inv_scale', C.c_float)]


class BatchDesc(C.Structure):
    """lfd_batch_desc_t"""
    _fields_ = [('src_offset', C.c_int64), ('src_pitch', C.c_int32), ('win_x0', C.c_int32), ('win_y0', C.c_int32),
                ('win_w', C.c_int32), ('win_h', C.c_int32), ('valid_w', C.c_int32), ('valid_h', C.c_int32),
                ('flip', C.c_int32), ('reserved_', C.c_int32)]


class PlanDesc(C.Structure):
    """lfd_plan_desc_t"""
    _fields_ = [('seed', C.c_uint64), ('resize_lo', C.c_double), ('resize_hi', C.c_double), ('resize_prob', C.c_double),
                ('flip_prob', C.c_double), ('arena_bytes', C.c_int64), ('epoch', C.c_uint32), ('batch', C.c_uint32),
                ('n', C.c_int32), ('num_images', C.c_int32), ('total_boxes', C.c_int32), ('crop_size', C.c_int32),
                ('c_src', C.c_int32), ('max_boxes_per_image', C.c_int32), ('max_boxes', C.c_int32), ('reserved_', C.c_int32)]


class PlanBufs(C.Structure):
    """lfd_plan_bufs_t"""
    _fields_ = [(k, C.c_void_p) for k in ('img_offset', 'img_h', 'img_w', 'box', 'label', 'box_offset', 'indices', 'desc', 'coef',
                                          'stage_box', 'stage_label', 'stage_count', 'boxes', 'labels', 'offsets', 'status')]


class EvalDesc(C.Structure):
    """lfd_eval_desc_t"""
    _fields_ = [('num_images', C.c_int32), ('num_categories', C.c_int32), ('num_gt', C.c_int32), ('det_capacity', C.c_int32),
                ('num_iou_thrs', C.c_int32), ('num_area_rngs', C.c_int32), ('num_rec_thrs', C.c_int32),
                ('num_max_dets', C.c_int32), ('max_dets', C.c_int32 * 8)]


class EvalBufs(C.Structure):
    """lfd_eval_bufs_t"""
    _fields_ = [(k, C.c_void_p) for k in ('det_box', 'det_score', 'det_img', 'det_cat', 'state', 'img_mask', 'gt_box', 'gt_area',
                                          'gt_crowd', 'gt_pair_start', 'iou_thrs', 'area_rng', 'rec_thrs', 'order', 'sort_key',
                                          'sorted_cat', 'sorted_rank', 'match_bits', 'ignore_bits', 'npig', 'cat_start',
                                          'precision', 'recall')]


class TT100KEvalDesc(C.Structure):
    """lfd_eval_tt100k_desc_t"""
    _fields_ = [(k, C.c_int32) for k in ('num_images', 'num_categories', 'num_gt', 'det_capacity', 'num_ious', 'num_minscores',
                                         'num_size_ranges', 'check_type', 'match_same')]


class TT100KEvalBufs(C.Structure):
    """lfd_eval_tt100k_bufs_t"""
    _fields_ = [(k, C.c_void_p) for k in ('det_box', 'det_score', 'det_img', 'det_cat', 'state', 'img_mask', 'gt_box', 'gt_cat',
                                          'gt_start', 'cat_in_types', 'ious', 'minscores', 'size_ranges', 'det_start', 'det_index',
                                          'det_match', 'gt_match', 'totals', 'per_category', 'det_code', 'gt_code')]


class WFEvalDesc(C.Structure):
    """lfd_eval_wf_desc_t"""
    _fields_ = [(k, C.c_int32) for k in ('num_images', 'num_gt', 'det_capacity', 'num_thresholds', 'as_written', 'label_index')] + [
        ('iou_thresh', C.c_double)]


class WFEvalBufs(C.Structure):
    """lfd_eval_wf_bufs_t"""
    _fields_ = [(k, C.c_void_p) for k in ('det_box', 'det_score', 'det_img', 'state', 'gt_box', 'gt_start', 'gt_kept', 'keep_len',
                                          'thr', 'det_start', 'det_index', 'det_gt', 'det_over', 'det_prop', 'det_rec', 'det_flags',
                                          'curve', 'faces', 'minmax')]


class RowsumJob(C.Structure):
    """lfd_rowsum_job_t"""
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('nrows', C.c_int32), ('row_stride', C.c_int32),
                ('count', C.c_int32), ('accumulate', C.c_int32)]


_P, _I64, _I32, _F, _SZ = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
_SIGNATURES = {
    'lfd_hip_abi_version': (C.c_int, []),
    'lfd_hip_status_string': (C.c_char_p, [C.c_int]),
    'lfd_hip_build_info': (C.c_char_p, []),
    'lfd_tuning_set': (C.c_int, [_I32, _I32]),
    'lfd_tuning_get': (_I32, [_I32]),
    'lfd_nms_cpu_f32': (C.c_int, [_P, _I64, _F, _P, _P]),
    'lfd_soft_nms_cpu_f32': (C.c_int, [_P, _I64, _F, _I32, _F, _F, _P, _P]),
    'lfd_nms_match_cpu_f32': (C.c_int, [_P, _I64, _F, _P, _P, _P]),
    'lfd_nms_cpu_f64': (C.c_int, [_P, _I64, _F, _P, _P]),
    'lfd_soft_nms_cpu_f64': (C.c_int, [_P, _I64, _F, _I32, _F, _F, _P, _P]),
    'lfd_nms_match_cpu_f64': (C.c_int, [_P, _I64, _F, _P, _P, _P]),
    'lfd_nms_workspace_bytes': (_SZ, [_I64]),
    'lfd_nms_f32': (C.c_int, [_P, _I64, _F, _P, _P, _P, _SZ, _P]),
    'lfd_batched_nms_workspace_bytes': (_SZ, [_I64]),
    'lfd_batched_nms_f32': (C.c_int, [_P, _P, _P, _I64, _F, _I32, _P, _P, _P, _P, _SZ, _P]),
    'lfd_detect_workspace_bytes': (_SZ, [C.POINTER(DetectDesc), _I32]),
    'lfd_detect_batched': (C.c_int, [C.POINTER(DetectDesc), _I32, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    'lfd_detect_ex_workspace_bytes': (_SZ, [C.POINTER(DetectDesc), _I32]),
    'lfd_detect_batched_ex': (C.c_int, [C.POINTER(DetectDesc), C.POINTER(DetectExt), _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _P,
                                        _P, _P, _SZ, _P]),
    'lfd_upsample_nearest_add_nhwc_f16': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    'lfd_relu_inplace_f16': (C.c_int, [_P, _I64, _P]),
    'lfd_maxpool3x3s2_nhwc_f16': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P]),
    'lfd_pack_level_outputs_f32': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P]),
    'lfd_upsample_nearest_add_bwd_nhwc_f16': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    'lfd_maxpool3x3s2_bwd_nhwc_f16': (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    'lfd_relu_bwd_add_f16': (C.c_int, [_P, _P, _P, _P, _I64, _P]),
    'lfd_bias_grad_workspace_bytes': (_SZ, []),
    'lfd_bias_grad_nhwc_f16': (C.c_int, [_P, _I64, _I32, _F, _P, _P, _SZ, _P]),
    'lfd_detect_workspace_reset': (C.c_int, [C.POINTER(DetectDesc), _I32, _P, _SZ, _P]),
    'lfd_detect_from_candidates': (C.c_int, [C.POINTER(DetectDesc), _I32, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    'lfd_decode_all': (C.c_int, [C.POINTER(DetectDesc), _I32, _P, _P, _I32, _P, _P, _P, _P]),
    'lfd_sigmoid_focal_loss_fwd': (C.c_int, [_P, _P, _I64, _I32, _F, _F, _P, _I32, _P]),
    'lfd_sigmoid_focal_loss_bwd': (C.c_int, [_P, _P, _P, _I64, _I32, _F, _F, _P, _I32, _P]),
    'lfd_reduce_workspace_bytes': (_SZ, []),
    'lfd_sigmoid_focal_loss_sum_f32': (C.c_int, [_P, _P, _I64, _I32, _F, _F, _P, _P, _SZ, _P]),
    'lfd_iou_loss_fwd_f32': (C.c_int, [_P, _P, _I64, _F, _P, _P]),
    'lfd_iou_loss_bwd_f32': (C.c_int, [_P, _P, _P, _I64, _F, _P, _P]),
    'lfd_bce_with_logits_f32': (C.c_int, [_P, _P, _I64, _P, _P, _P]),
    'lfd_quality_focal_loss_f32': (C.c_int, [_P, _P, _P, _I64, _I32, _F, _P, _P, _P]),
    'lfd_pointwise_loss_f32': (C.c_int, [_P, _P, _I64, _I32, _F, _P, _P, _P]),
    'lfd_box_loss_f32': (C.c_int, [_P, _P, _I64, _I32, _F, _P, _P, _P]),
    'lfd_assign_targets_f32': (C.c_int, [C.POINTER(AssignDesc), _P, _P, _P, _P, _P, _P]),
    'lfd_cross_entropy_fwd_f32': (C.c_int, [_P, _P, _I64, _I32, _P, _P]),
    'lfd_cross_entropy_bwd_f32': (C.c_int, [_P, _P, _P, _I64, _I32, _P, _P]),
    'lfd_get_loss_workspace_bytes': (_SZ, []),
    'lfd_get_loss_sums_f32': (C.c_int, [C.POINTER(LossDesc), _P, _P, _P, _P, _P, _SZ, _P, _P]),
    'lfd_get_loss_finalize_f32': (C.c_int, [C.POINTER(LossDesc), _P, _P, _F, _P, _P]),
    'lfd_get_loss_bwd_f32': (C.c_int, [C.POINTER(LossDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_get_loss_ex_workspace_bytes': (_SZ, []),
    'lfd_get_loss_ex_sums_f32': (C.c_int, [C.POINTER(LossDescEx), _P, _P, _P, _P, _P, _SZ, _P, _P]),
    'lfd_get_loss_ex_finalize_f32': (C.c_int, [C.POINTER(LossDescEx), _P, _P, _F, _P, _P]),
    'lfd_get_loss_ex_bwd_f32': (C.c_int, [C.POINTER(LossDescEx), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_assign_targets_fcos_f32': (C.c_int, [C.POINTER(AssignFcosDesc), _P, _P, _I64, _P, _P, _P, _P, _P]),
    'lfd_assign_targets_v2_f32': (C.c_int, [C.POINTER(AssignDesc), _P, _P, _I64, _P, _P, _P, _P, _P]),
    'lfd_fcos_loss_workspace_bytes': (_SZ, []),
    'lfd_fcos_loss_sums_f32': (C.c_int, [C.POINTER(FcosLossDesc), _P, _P, _P, _P, _P, _P, _SZ, _P, _P]),
    'lfd_fcos_loss_finalize_f32': (C.c_int, [C.POINTER(FcosLossDesc), _P, _P, _F, _P, _P]),
    'lfd_fcos_loss_bwd_f32': (C.c_int, [C.POINTER(FcosLossDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_grad_norm_workspace_bytes': (_SZ, []),
    'lfd_grad_norm_clip_coef_f32': (C.c_int, [_P, _I64, _F, _P, _P, _SZ, _P, _P, _P]),
    'lfd_scale_by_clip_coef_f32': (C.c_int, [_P, _I64, _P, _P]),
    'lfd_sgd_step_f32': (C.c_int, [_P, _P, _P, _I64, _F, _F, _F, _F, _I32, _I32, _P, _I32, _I32, _P]),
    'lfd_train_workspace_bytes': (_SZ, []),
    'lfd_bn_train_stats_f16': (C.c_int, [_P, _I64, _I32, _F, _F, _P, _P, _P, _SZ, _P, _P]),
    'lfd_conv2d_bn_stats_nhwc_f16': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _SZ, _P, _P]),
    'lfd_conv1x1_of_bn_relu_bn_stats_nhwc_f16': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _SZ, _P, _P]),
    'lfd_bn_train_apply_f16': (C.c_int, [_P, _I64, _I32, _P, _P, _P, _P, _I32, _P, _P]),
    'lfd_bn_train_bwd_f16': (C.c_int, [_P, _P, _P, _I32, _I64, _I32, _P, _P, _P, _F, _I32, _P, _SZ, _P, _P, _P, _P, _P]),
    'lfd_pack_conv_weights_train_f16': (C.c_int, [_P, _I32, _I32, _P]),
    'lfd_pack_conv_weight_train_f16': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    'lfd_gn_train_stats_f16': (C.c_int, [_P, _I32, _I64, _I32, _I32, _F, _P, _SZ, _P, _P]),
    'lfd_gn_train_apply_f16': (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _P, _P, _I32, _P, _P]),
    'lfd_gn_train_stats_apply_f16': (C.c_int, [_P, _I32, _I64, _I32, _I32, _F, _P, _P, _I32, _P, _SZ, _P, _P, _P]),
    'lfd_gn_train_stats_apply_seg_f16': (C.c_int, [_P, _I32, _I32, _P, _I32, _I32, _F, _P, _P, _I32, _P, _SZ, _P, _P, _P]),
    'lfd_gn_train_bwd_seg_f16': (C.c_int, [_P, _P, _P, _I32, _I32, _P, _I32, _I32, _P, _P, _F, _I32, _P, _SZ, _P, _P, _P, _P]),
    'lfd_bn_train_apply_into_f16': (C.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _P, _I64, _I64, _P]),
    'lfd_bn_train_bwd_from_f16': (C.c_int, [_P, _I64, _I64, _P, _I32, _I32, _I64, _I32, _P, _P, _P, _F, _I32, _P, _SZ, _P, _P, _P, _P]),
    'lfd_head_out_split_concat_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _P]),
    'lfd_head_out_grad_concat_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _F, _P, _P, _SZ, _P]),
    'lfd_conv2d_bn_partials_nhwc_f16': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _SZ, C.POINTER(C.c_int32), _P]),
    'lfd_bn_train_finish_into_levels_f16': (C.c_int, [C.POINTER(BnFwdLevel), _I32, _I32, _I32, _P, _I64, _P]),
    'lfd_bn_train_bwd_from_levels_f16': (C.c_int, [_P, _I64, C.POINTER(BnBwdLevel), _I32, _I32, _I32, _F, _I32, _P, _SZ, _P]),
    'lfd_head_out_split_levels_f16': (C.c_int, [_P, _I32, _I64, C.POINTER(HeadOutLevel), _I32, _P]),
    'lfd_head_out_grad_levels_f16': (C.c_int, [_P, _I32, _I64, C.POINTER(HeadOutLevel), _I32, _F, _P, _P, _SZ, _P]),
    'lfd_gn_train_bwd_f16': (C.c_int, [_P, _P, _P, _I32, _I64, _I32, _I32, _P, _P, _F, _I32, _P, _SZ, _P, _P, _P, _P]),
    'lfd_zero_insert2_nhwc_f16': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    'lfd_conv3x3s2_dgrad_nhwc_f16': (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P]),
    'lfd_conv_wgrad_nhwc_f16': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P, _SZ, _P, _P]),
    'lfd_conv_wgrad_partial_rows': (_I32, [_I32, _I32, _I32, _I32, _I32, _I32, _I32]),
    'lfd_conv_wgrad_partials_nhwc_f16': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _SZ, _P]),
    'lfd_conv1x1_wgrad_partials_of_bn_relu_f16': (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _SZ, _P]),
    'lfd_wgrad_final_batched_f32': (C.c_int, [_P, _I32, _I32, _P]),
    'lfd_rows_sum_batched_f32': (C.c_int, [_P, _I32, _P]),
    'lfd_stem_conv0_train_fwd': (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'lfd_head_out_split_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _P]),
    'lfd_head_out_grad_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _F, _P, _P, _SZ, _P]),
    # ... for an output conv padded to `rows` in {64, 128} output rows (csrc/head_out_wide.hip; 64 forwards to the ones above)
    'lfd_head_out_split_w_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _I32, _P]),
    'lfd_head_out_grad_w_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _I32, _F, _P, _P, _SZ, _P]),
    'lfd_head_out_split_concat_w_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _I32, _P]),
    'lfd_head_out_grad_concat_w_f16': (C.c_int, [_P, _I32, _I32, _I64, _I64, C.POINTER(HeadOutSeg), _I32, _I32, _F, _P, _P, _SZ, _P]),
    'lfd_head_out_split_levels_w_f16': (C.c_int, [_P, _I32, _I64, C.POINTER(HeadOutLevel), _I32, _I32, _P]),
    'lfd_head_out_grad_levels_w_f16': (C.c_int, [_P, _I32, _I64, C.POINTER(HeadOutLevel), _I32, _I32, _F, _P, _P, _SZ, _P]),
    # the glue around FCOSHead's output convs, all levels in one launch (csrc/fcos_out.hip)
    'lfd_fcos_out_grad_workspace_bytes': (_SZ, [_I32, _I32]),
    'lfd_fcos_out_pack_levels_f32': (C.c_int, [C.POINTER(FcosOutLevel), _I32, _I32, _I32, _I32, _I64, _P, _P, _P, _P]),
    'lfd_fcos_out_grad_levels_f32': (C.c_int, [C.POINTER(FcosOutLevel), _I32, _I32, _I32, _I32, _I64, _P, _P, _P, _P, _F, _P, _P, _P,
                                               _P, _SZ, _P]),
    # the glue around LFDHead's fp32-logit output convs, all levels and both convs in one launch (csrc/lfd_out.hip)
    'lfd_lfdhead_out_grad_workspace_bytes': (_SZ, [_I32, _I32]),
    'lfd_lfdhead_out_pack_levels_f32': (C.c_int, [C.POINTER(LfdHeadOutLevel), _I32, _I32, _I32, _I32, _I64, _P, _P, _P]),
    'lfd_lfdhead_out_grad_levels_f32': (C.c_int, [C.POINTER(LfdHeadOutLevel), _I32, _I32, _I32, _I32, _I64, _P, _P, _F, _P, _SZ, _P]),
    'lfd_stem_conv0_train_fwd_bn_stats': (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _F, _F, _P, _P, _P, _SZ, _P, _P]),
    'lfd_stem_conv0_wgrad': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _F, _I32, _P, _SZ, _P, _P]),
    'lfd_stem_conv0_bn_bwd_wgrad': (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _F, _I32, _P, _SZ, _P, _P, _P, _P]),
    'lfd_stem_conv0_bn_bwd_wgrad_rows': (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _F, _I32, _I32, _P, _SZ, _P, _P, _P, _P]),
    'lfd_bn_eval_stats_f32': (C.c_int, [_P, _I32, _I32, _P]),
    'lfd_conv_bn_eval_fold_f32': (C.c_int, [_P, _I32, _I32, _P]),
    'lfd_bn_eval_bwd_f16': (C.c_int, [_P, _P, _P, _I32, _I64, _I32, _P, _P, _P, _F, _I32, _P, _SZ, _P, _P, _P, _P, _P]),
    'lfd_bn_train_bwd_rows_f16': (C.c_int, [_P, _P, _I64, _I32, _P, _P, _P, _F, _I32, _I32, _P, _SZ, _P, _P, _P, _P]),
    'lfd_conv1x1_dgrad_bn_bwd_sums_nhwc_f16': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, C.POINTER(C.c_int32), _P]),
    'lfd_stem_gray_train_fwd': (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'lfd_stem_gray_train_fwd_bn_stats': (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _F, _F, _P, _P, _P, _SZ, _P, _P]),
    'lfd_stem_gray_wgrad': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _F, _I32, _P, _SZ, _P, _P]),
    'lfd_stem_gray_bn_bwd_wgrad_rows': (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _F, _I32, _I32, _P, _SZ, _P, _P, _P, _P]),
    'lfd_stem_conv_f16': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    'lfd_stem_gray_f16': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    'lfd_stem7_conv_f16': (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    'lfd_stem7_packed_weight_halfs': (_SZ, []),
    'lfd_pl_stem_gray_pair': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P]),
    'lfd_stem_faster_fused_f16': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_head_partial_floats': (_SZ, [C.POINTER(HeadDesc)]),
    'lfd_head_forward_f16': (C.c_int, [C.POINTER(HeadDesc), _I32, C.POINTER(HeadLevelPtrs), _P, _P, _P, _P, _P, _P, _P]),
    'lfd_head_forward_wide_f16': (C.c_int, [C.POINTER(HeadDesc), C.POINTER(HeadLevelPtrs), _P, _P, _P, _P, _P, _P]),
    'lfd_head_forward_decode_f16': (C.c_int, [C.POINTER(HeadDesc), C.POINTER(HeadLevelPtrs), _P, _P, _P, _P, _P,
                                              C.POINTER(DetectDesc), _P, _P, _SZ, _P]),
    'lfd_groupnorm_finalize': (C.c_int, [C.POINTER(HeadDesc), _P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _F, _P, _P]),
    'lfd_groupnorm_finalize_fold': (C.c_int, [C.POINTER(HeadDesc), _P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _F, _P,
                                              C.POINTER(HeadLevelPtrs), _I32, _P]),
    'lfd_conv_packed_weight_halfs': (_SZ, [_I32, _I32, _I32]),
    'lfd_conv2d_nhwc_f16_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'lfd_conv2d_nhwc_f16': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_fasterblock_fused_f16': (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_fasterblock128_fused_f16': (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_downblock_fused_f16': (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_conv2d_nhwc_f16_acc32': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P]),
    'lfd_conv256_nhwc_f16_supported': (C.c_int, [_I32, _I32, _I32, _I32]),
    'lfd_conv256_nhwc_f16': (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    'lfd_conv2d_nhwc_i8_supported': (C.c_int, [_I32, _I32, _I32, _I32]),
    'lfd_conv2d_nhwc_i8': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, C.c_float, _P, _P, C.c_float, _P]),
    'lfd_quantize_nhwc_f16_i8': (C.c_int, [_P, _P, _I64, C.c_float, _P]),
    'lfd_quantize_pad_nhwc_f16_i8': (C.c_int, [_P, _P, _I64, _I32, _I32, C.c_float, _P]),
    'lfd_block_i8_fused': (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P, C.c_float, _P]),
    'lfd_block128_i8_fused': (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P, C.c_float, _P]),
    'lfd_conv2d_downsample_nhwc_i8_supported': (C.c_int, [_I32, _I32]),
    'lfd_conv2d_downsample_nhwc_i8': (C.c_int, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_entry_i8_fused': (C.c_int, [_I32, _I32, _I32, _I32, _I32, _P, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P,
                                     _P]),
    'lfd_entry_i8_fused_supported': (C.c_int, [_I32, _I32]),
    'lfd_stem_conv_i8': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, C.c_float, _P, _P]),
    'lfd_stem_conv_i8_supported': (C.c_int, [_I32, _I32, _I32]),
    'lfd_stem_faster_fused_i8': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P]),
    'lfd_stem_faster_fused_i8_supported': (C.c_int, [_I32, _I32]),
    'lfd_abs_histogram_f16': (C.c_int, [_P, _I64, _I32, _I32, _P, _P]),
    'lfd_p32_conv_packed_weight_halfs': (_SZ, [_I32, _I32, _I32]),
    'lfd_p32_conv2d_nhwc_f32': (C.c_int, [C.POINTER(P32ConvDesc), _P, _P, _P, _P, _P, _P, _P]),
    'lfd_p32_conv2d_tail_nhwc_f32': (C.c_int, [C.POINTER(P32ConvDesc), _P, _P, _P, _P, _P, _P, _I32, _P]),
    'lfd_p32_conv2d_merge_nhwc_f32': (C.c_int, [C.POINTER(P32ConvDesc), _P, _P, _P, _P, _P, _I32, _I32, _P]),
    'lfd_p32_upsample_nearest_add_f32': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    'lfd_p32_relu_f32': (C.c_int, [_P, _I64, _P]),
    'lfd_p32_maxpool3x3s2_f32': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P]),
    'lfd_p32_exp_rows_f32': (C.c_int, [_P, _I32, _I64, _I64, _I64, _I32, _P]),
    'lfd_pl_stem_pair': (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P]),
    'lfd_pl_stem2x': (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P]),
    'lfd_pl_conv2d': (C.c_int, [C.POINTER(PlConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_pl_block64': (C.c_int, [_I32, _I32, _I32, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P]),
    'lfd_pl_conv2d_levels': (C.c_int, [C.POINTER(PlConvDesc), C.POINTER(PlLevel), _I32, _P, _P]),
    'lfd_pl_head_levels': (C.c_int, [C.POINTER(PlHeadDesc), C.POINTER(PlHeadLevel), _I32, _P, _P]),
    'lfd_pl_groupnorm_relu': (C.c_int, [_P, _I64, _I32, _I64, _I32, _P, _P, _P, _F, _I32, _P]),
    'lfd_p32_groupnorm_workspace_bytes': (_SZ, [_I32, _I32]),
    'lfd_p32_groupnorm_relu_f32': (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _P, _F, _I32, _P, _SZ, _P]),
    'lfd_conv2d_downsample_nhwc_f16': (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'lfd_batch_assemble_f32': (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    'lfd_plan_bbox_crop_batch': (C.c_int, [C.POINTER(PlanDesc), C.POINTER(PlanBufs), _P]),
    'lfd_eval_append_dets_f32': (C.c_int, [C.POINTER(EvalDesc), C.POINTER(EvalBufs), _P, _P, _P, _I32, _I32, _P, _I32, _P, _I32, _P]),
    'lfd_eval_append_rows_f64': (C.c_int, [C.POINTER(EvalDesc), C.POINTER(EvalBufs), _P, _I64, _P, _I32, _P]),
    'lfd_eval_match_workspace_bytes': (_SZ, [C.POINTER(EvalDesc)]),
    'lfd_eval_match': (C.c_int, [C.POINTER(EvalDesc), C.POINTER(EvalBufs), _P, _SZ, _P]),
    'lfd_eval_accumulate_workspace_bytes': (_SZ, [C.POINTER(EvalDesc)]),
    'lfd_eval_accumulate': (C.c_int, [C.POINTER(EvalDesc), C.POINTER(EvalBufs), _P, _SZ, _P]),
    'lfd_eval_tt100k_append_dets_f32': (C.c_int, [C.POINTER(TT100KEvalDesc), C.POINTER(TT100KEvalBufs), _P, _P, _P, _I32, _I32, _P, _I32,
                                                  _P, _P]),
    'lfd_eval_tt100k_append_rows_f64': (C.c_int, [C.POINTER(TT100KEvalDesc), C.POINTER(TT100KEvalBufs), _P, _I64, _P, _I32, _P]),
    'lfd_eval_tt100k_workspace_bytes': (_SZ, [C.POINTER(TT100KEvalDesc)]),
    'lfd_eval_tt100k_match': (C.c_int, [C.POINTER(TT100KEvalDesc), C.POINTER(TT100KEvalBufs), _P, _SZ, _P]),
    'lfd_eval_wf_append_dets_f32': (C.c_int, [C.POINTER(WFEvalDesc), C.POINTER(WFEvalBufs), _P, _P, _P, _I32, _I32, _P, _P]),
    'lfd_eval_wf_append_rows_f64': (C.c_int, [C.POINTER(WFEvalDesc), C.POINTER(WFEvalBufs), _P, _I64, _P]),
    'lfd_eval_wf_workspace_bytes': (_SZ, [C.POINTER(WFEvalDesc)]),
    'lfd_eval_wf_match': (C.c_int, [C.POINTER(WFEvalDesc), C.POINTER(WFEvalBufs), _P, _SZ, _P]),
}


# lfd_tune_key_t (include/lfd_hip.h) and the environment names rounds 1-3 used for the same switches: the LIBRARY reads no
# environment variable any more; this host layer applies them once, explicitly, when it loads the library (tests and the A/B
# tools that start a fresh interpreter per variant keep working), and `tune()` sets a knob at run time.
TUNE_KEYS = {'HEAD2': 0, 'H2_CHUNK': 1, 'H2_AGPR': 2, 'H2_A1': 3, 'STEM2X': 4, 'X2_ALN': 5, 'X2_STAGGER': 6, 'BLOCK_ROWS': 7,
             'ROWS_WGS': 8, 'CONV128_SPLITK': 9, 'CONV0_VALU': 10, 'PL_C3': 11, 'PL_HEAD_OUT_REGS': 12, 'PL_HEAD_ROLES': 13, 'PL_STEM': 14}


def tune(name, value=None):
    """tune('BLOCK_ROWS', 0) -> previous value; tune('BLOCK_ROWS') -> current value (lfd_tuning_set / lfd_tuning_get)"""
    key = TUNE_KEYS[name]
    prev = lib().lfd_tuning_get(key)
    if value is not None:
        check(lib().lfd_tuning_set(key, int(value)), 'lfd_tuning_set')
    return prev


def declared_symbols():
    return sorted(_SIGNATURES)


def lib():
    """Loads liblfd_hip.so (after torch, so that the HIP runtime already mapped by torch is
    the one the kernels register with -- same soname libamdhip64.so.7)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'liblfd_hip.so not found at %s -- build it with `python __graft_entry__.py` '
                '(hipcc --offload-arch=gfx950); lfd_amd has no CPU/PyTorch fallback.' % LIB_PATH)
        import torch  # noqa: F401  (maps the HIP runtime first)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)   # AttributeError -> missing export: loud by design
            fn.restype, fn.argtypes = res, args
        if l.lfd_hip_abi_version() != ABI_VERSION:
            raise RuntimeError('liblfd_hip.so ABI version mismatch: %s reports %d, this package binds version %d '
                               '(struct layouts differ -- rebuild with `python __graft_entry__.py`)'
                               % (LIB_PATH, l.lfd_hip_abi_version(), ABI_VERSION))
        for name, key in TUNE_KEYS.items():
            v = os.environ.get('LFD_' + name)
            if v is not None and v.strip().lstrip('-').isdigit():
                l.lfd_tuning_set(key, int(v))
        _lib = l
    return _lib


def check(status, what):
    if status != 0:
        raise RuntimeError('%s failed: %s (status %d)' % (what, lib().lfd_hip_status_string(status).decode(), status))


def require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError('%s: lfd_amd kernels run on the MI355X only (got a %s tensor); '
                           'there is no CPU implementation' % (what, t.device))


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
