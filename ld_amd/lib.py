"""ctypes binding of libldhip.so (C ABI declared in include/ld_hip.h).

There is no fallback: if the shared library is missing, or a tensor handed to
an op is not a contiguous fp32/int64 tensor on a HIP device, the call raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, '_lib', 'libldhip.so')

LD_MAX_LEVELS = 8
LD_NUM_LOSS_KEYS = 8
LD_SGD_MAX_CLASSES = 64  # ld_sgd_step_classes: parameter classes per table
LOSS_KEYS = ('loss_cls', 'loss_bbox', 'loss_dfl', 'loss_ld', 'loss_ld_vlr',
             'loss_kd', 'loss_kd_neg', 'loss_im')


class LdError(RuntimeError):
    pass


class LevelT(C.Structure):
    _fields_ = [('H', C.c_int32), ('W', C.c_int32), ('stride', C.c_int32),
                ('offset', C.c_int32)]


class GeomT(C.Structure):
    _fields_ = [('num_levels', C.c_int32), ('num_anchors', C.c_int32),
                ('num_imgs', C.c_int32), ('anchor_scale', C.c_int32),
                ('lv', LevelT * LD_MAX_LEVELS)]


class MapsT(C.Structure):
    _fields_ = [('ptr', C.c_void_p * LD_MAX_LEVELS),
                ('stride_n', C.c_int64 * LD_MAX_LEVELS),
                ('stride_c', C.c_int64 * LD_MAX_LEVELS)]


class LossHpT(C.Structure):
    _fields_ = [('num_classes', C.c_int32), ('reg_max', C.c_int32),
                ('topk', C.c_int32), ('feat_channels', C.c_int32),
                ('lw_cls', C.c_float), ('qfl_beta', C.c_float),
                ('lw_bbox', C.c_float), ('giou_eps', C.c_float),
                ('lw_dfl', C.c_float), ('lw_ld', C.c_float),
                ('T_ld', C.c_float), ('lw_ld_vlr', C.c_float),
                ('T_ld_vlr', C.c_float), ('lw_kd', C.c_float),
                ('T_kd', C.c_float), ('lw_im', C.c_float),
                ('cls_channels', C.c_int32), ('flags', C.c_int32),
                ('lw_ctr', C.c_float), ('focal_alpha', C.c_float)]


class DeltaT(C.Structure):  # ld_delta_t
    _fields_ = [('means', C.c_float * 4), ('stds', C.c_float * 4),
                ('max_ratio', C.c_float), ('beta', C.c_float),
                ('num_base', C.c_int32), ('box_term', C.c_int32)]


LD_LOSS_PROB_CLS = 1
LD_IM_CENTER_INSIDE = 2
LD_LOSS_ATSS = 4
LD_LOSS_FCOS = 8
LD_LOSS_RETINA = 16
LD_LOSS_DELTA = 32
LD_LOSS_DIST = 64
LD_LOSS_DIST_NORM = 128
LD_DELTA_TERMS = {'decoded': 0, 'l1': 1, 'smooth_l1': 2}
LD_LOSS_PART_CLS = 4
LD_LOSS_BBOX_SHIFT = 8
LD_LOSS_BBOX_MODES = {'giou': 0, 'iou': 1, 'iou_linear': 2, 'diou': 3,
                      'ciou': 4}
LD_INFER_VOTING = 1
LD_INFER_PROB = 2
LD_INFER_POINTS = 4
LD_INFER_DELTA = 16
LD_INFER_DIST = 32
LD_SCALE_ACT_MODES = {'exp': 0, 'relu': 1, 'relu_stride': 2}
LD_AUG_RESCALE = 8
LD_MAX_AUG_VIEWS = 16
LD_FLIP = {None: 0, 'horizontal': 1, 'vertical': 2, 'diagonal': 3}


class AugViewT(C.Structure):
    _fields_ = [('boxes', C.c_void_p), ('scores', C.c_void_p),
                ('factors', C.c_void_p), ('K', C.c_int32),
                ('score_stride', C.c_int32), ('flip', C.c_int32),
                ('reserved', C.c_int32), ('img_h', C.c_float),
                ('img_w', C.c_float), ('scale_factor', C.c_float * 4)]


LD_EVAL_MAX_SCALES = 16
LD_EVAL_MAX_THRS = 16
LD_EVAL_11POINTS = 1
LD_EVAL_IMAGE_NO_LDS = 1
LD_EVAL_RECALLS_MAX_NUMS = 16
LD_EVAL_RECALLS_NO_LDS = 1
LD_LEVELS_MIX_MAX_K = 16


class EvalBatchT(C.Structure):
    _fields_ = [('dets', C.c_void_p), ('det_labels', C.c_void_p),
                ('det_off', C.c_void_p), ('gts', C.c_void_p),
                ('gt_labels', C.c_void_p), ('gt_off', C.c_void_p),
                ('ign', C.c_void_p), ('ign_labels', C.c_void_p),
                ('ign_off', C.c_void_p), ('num_imgs', C.c_int32),
                ('num_dets', C.c_int32), ('num_gts', C.c_int32),
                ('num_ign', C.c_int32)]


LD_COCO_MAX_THRS = 16
LD_COCO_MAX_AREAS = 4
LD_COCO_MAX_MAXDETS = 4
LD_COCO_MAX_REC_THRS = 128
LD_COCO_MAX_CELL_GTS = 1024


class CocoBatchT(C.Structure):
    _fields_ = [('dets', C.c_void_p), ('labels', C.c_void_p),
                ('det_off', C.c_void_p), ('img_rank', C.c_void_p),
                ('label_cat', C.c_void_p), ('gt_box', C.c_void_p),
                ('gt_area', C.c_void_p), ('gt_crowd', C.c_void_p),
                ('gt_id', C.c_void_p), ('gt_cell_off', C.c_void_p),
                ('num_imgs', C.c_int32), ('num_dets', C.c_int32),
                ('num_labels', C.c_int32), ('max_img_dets', C.c_int32),
                ('num_all_imgs', C.c_int32), ('num_cats', C.c_int32),
                ('num_gts', C.c_int32), ('max_cell_gts', C.c_int32)]


class CocoErrBatchT(C.Structure):  # ld_coco_err_batch_t
    _fields_ = [('dets', C.c_void_p), ('labels', C.c_void_p),
                ('det_off', C.c_void_p), ('img_rank', C.c_void_p),
                ('label_cat', C.c_void_p), ('gt_box', C.c_void_p),
                ('gt_area', C.c_void_p), ('gt_crowd', C.c_void_p),
                ('gt_id', C.c_void_p), ('gt_cat', C.c_void_p),
                ('gt_img_off', C.c_void_p), ('cat_sup', C.c_void_p),
                ('num_imgs', C.c_int32), ('num_dets', C.c_int32),
                ('num_labels', C.c_int32), ('max_img_dets', C.c_int32),
                ('num_all_imgs', C.c_int32), ('num_cats', C.c_int32),
                ('num_gts', C.c_int32), ('max_img_gts', C.c_int32)]


class ConvLevelT(C.Structure):
    _fields_ = [('Hin', C.c_int32), ('Win', C.c_int32), ('Hout', C.c_int32),
                ('Wout', C.c_int32), ('off_in', C.c_int32),
                ('off_out', C.c_int32)]


class ConvT(C.Structure):
    _fields_ = [('N', C.c_int32), ('Cin', C.c_int32), ('Cout', C.c_int32),
                ('KH', C.c_int32), ('KW', C.c_int32), ('stride', C.c_int32),
                ('pad', C.c_int32), ('num_levels', C.c_int32),
                ('Pin', C.c_int32), ('Pout', C.c_int32),
                ('lv', ConvLevelT * LD_MAX_LEVELS)]


class WtJobT(C.Structure):  # ld_wt_job_t
    _fields_ = [('w', C.c_void_p), ('wt_fwd', C.c_void_p),
                ('wt_bwd', C.c_void_p), ('Cout', C.c_int32),
                ('Cin', C.c_int32), ('ntaps', C.c_int32),
                ('first_block', C.c_int32)]


class WgradJobT(C.Structure):  # ld_wgrad_job_t
    _fields_ = [('slabs', C.c_void_p), ('dw', C.c_void_p),
                ('splits', C.c_int32), ('ntaps', C.c_int32),
                ('Cout', C.c_int32), ('Cin', C.c_int32),
                ('accumulate', C.c_int32), ('first_block', C.c_int32)]


class BnFinJobT(C.Structure):  # ld_bn_fin_job_t
    _fields_ = [('partial', C.c_void_p), ('dgamma', C.c_void_p),
                ('dbeta', C.c_void_p), ('C', C.c_int32), ('nsplit', C.c_int32),
                ('accumulate', C.c_int32), ('first_block', C.c_int32)]


LD_GRAD_DEFER = 2


class BottleneckT(C.Structure):  # ld_bottleneck_t
    _fields_ = [('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('Cin', C.c_int32), ('mid', C.c_int32), ('reserved', C.c_int32),
                ('w1', C.c_void_p), ('w2', C.c_void_p), ('w3', C.c_void_p),
                ('scale1', C.c_void_p), ('shift1', C.c_void_p),
                ('scale2', C.c_void_p), ('shift2', C.c_void_p),
                ('scale3', C.c_void_p), ('shift3', C.c_void_p)]


class BnJobT(C.Structure):  # ld_bn_job_t
    _fields_ = [('gamma', C.c_void_p), ('beta', C.c_void_p),
                ('mean', C.c_void_p), ('var', C.c_void_p),
                ('scale', C.c_void_p), ('shift', C.c_void_p),
                ('rstd', C.c_void_p), ('eps', C.c_float), ('C', C.c_int32),
                ('first_block', C.c_int32), ('reserved', C.c_int32)]


class ImageT(C.Structure):  # ld_image_t
    _fields_ = [('data', C.c_void_p), ('src_h', C.c_int32),
                ('src_w', C.c_int32), ('new_h', C.c_int32),
                ('new_w', C.c_int32), ('flip', C.c_int32),
                ('reserved', C.c_int32)]


class ImageAugT(C.Structure):  # ld_image_aug_t
    _fields_ = [('data', C.c_void_p), ('src_h', C.c_int32),
                ('src_w', C.c_int32), ('canvas_h', C.c_int32),
                ('canvas_w', C.c_int32), ('img_top', C.c_int32),
                ('img_left', C.c_int32), ('win_y', C.c_int32),
                ('win_x', C.c_int32), ('win_h', C.c_int32),
                ('win_w', C.c_int32), ('new_h', C.c_int32),
                ('new_w', C.c_int32), ('crop_y', C.c_int32),
                ('crop_x', C.c_int32), ('out_h', C.c_int32),
                ('out_w', C.c_int32), ('flip', C.c_int32),
                ('fill', C.c_uint8 * 4)]


class ImagePhotoT(C.Structure):  # ld_image_photo_t
    _fields_ = [('data', C.c_void_p), ('src_h', C.c_int32),
                ('src_w', C.c_int32), ('canvas_h', C.c_int32),
                ('canvas_w', C.c_int32), ('img_top', C.c_int32),
                ('img_left', C.c_int32), ('win_y', C.c_int32),
                ('win_x', C.c_int32), ('win_h', C.c_int32),
                ('win_w', C.c_int32), ('new_h', C.c_int32),
                ('new_w', C.c_int32), ('crop_y', C.c_int32),
                ('crop_x', C.c_int32), ('out_h', C.c_int32),
                ('out_w', C.c_int32), ('flip', C.c_int32),
                ('fill', C.c_float * 3), ('delta', C.c_float),
                ('alpha', C.c_float), ('saturation', C.c_float),
                ('hue', C.c_float), ('do_brightness', C.c_int32),
                ('do_contrast', C.c_int32), ('contrast_mode', C.c_int32),
                ('do_saturation', C.c_int32), ('do_hue', C.c_int32),
                ('do_hsv', C.c_int32), ('perm', C.c_int32 * 3),
                ('reserved', C.c_int32)]


class JpegInfoT(C.Structure):  # ld_jpeg_info_t
    _fields_ = [('width', C.c_int32), ('height', C.c_int32),
                ('ncomp', C.c_int32), ('hmax', C.c_int32), ('vmax', C.c_int32),
                ('restart_interval', C.c_int32), ('mcus_x', C.c_int32),
                ('mcus_y', C.c_int32), ('h', C.c_int32 * 4),
                ('v', C.c_int32 * 4), ('tq', C.c_int32 * 4),
                ('blocks_w', C.c_int32 * 4), ('blocks_h', C.c_int32 * 4),
                ('plane_w', C.c_int32 * 4), ('plane_h', C.c_int32 * 4),
                ('coef_off', C.c_int64 * 4), ('coef_count', C.c_int64),
                ('coef_bytes', C.c_int64), ('quant', (C.c_uint16 * 64) * 4),
                ('message', C.c_char * 64)]


class ConvEpilogueT(C.Structure):
    _fields_ = [('bias', C.c_void_p), ('scale', C.c_void_p),
                ('shift', C.c_void_p), ('residual', C.c_void_p),
                ('relu', C.c_int32), ('reserved', C.c_int32),
                ('y_c8', C.c_void_p), ('residual_c8', C.c_void_p),
                ('y_raw', C.c_void_p), ('y_raw_c8', C.c_void_p)]


class LevelsT(C.Structure):
    _fields_ = [('num_levels', C.c_int32), ('H', C.c_int32 * LD_MAX_LEVELS),
                ('W', C.c_int32 * LD_MAX_LEVELS)]


_lib = None


def lib_available():
    return os.path.exists(LIB_PATH)


def get_lib():
    """Load libldhip.so (once).  Raises LdError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LdError(
            f'{LIB_PATH} not found: the HIP extension has not been built '
            '(run `python -m ld_amd.build`); ld_amd has no fallback path')
    lib = C.CDLL(LIB_PATH)
    _declare(lib)
    if lib.ld_abi_version() != ABI_VERSION:
        raise LdError('libldhip.so ABI version mismatch; rebuild')
    _load_tune_tables(lib)
    _lib = lib
    return lib


TUNE_TABLE = os.path.join(_HERE, 'tune', 'gfx950.txt')


def _load_tune_tables(lib):
    """Conv tile shapes: the table shipped in-tree (picked on an MI355X), then
    LD_CONV_TUNE_FILE on top of it.  With the same tables every process and
    every rank launches the same shapes, so results are bit-reproducible; a
    geometry in neither falls back to a deterministic model inside the
    library.  Timing new geometries is explicit: ld_amd.layers.autotune()."""
    if os.environ.get('LD_CONV_TUNE_TABLE', '1') != '0' and \
            os.path.exists(TUNE_TABLE):
        lib.ld_conv_tune_load(TUNE_TABLE.encode())
    extra = os.environ.get('LD_CONV_TUNE_FILE')
    if extra and os.path.exists(extra):
        lib.ld_conv_tune_load(extra.encode())


def save_tune_table(path):
    return get_lib().ld_conv_tune_save(str(path).encode())


ABI_VERSION = 26
_vp, _i64, _i32, _f32, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_size_t
_G, _H, _M = C.POINTER(GeomT), C.POINTER(LossHpT), C.POINTER(MapsT)
_CV, _EP, _LV = C.POINTER(ConvT), C.POINTER(ConvEpilogueT), C.POINTER(LevelsT)
_AV = C.POINTER(AugViewT)
_D = C.POINTER(DeltaT)

# name -> (restype, argtypes); kept in one table so the CPU test-suite can
# check that every symbol include/ld_hip.h declares is exported.
SIGNATURES = {
    'ld_abi_version': (C.c_int, []),
    'ld_target_arch': (C.c_char_p, []),
    'ld_atss_targets_workspace_bytes': (_sz, [_G, _i32]),
    'ld_atss_targets': (C.c_int, [_G, _H, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_atss_targets_ex': (C.c_int, [_G, _H, _vp, _vp, _vp, _vp, _i32, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _sz, _vp]),
    'ld_grid_anchors': (C.c_int, [_G, _vp, _vp]),
    'ld_loss_workspace_bytes': (_sz, [_G]),
    'ld_fcos_targets': (C.c_int, [_G, _i32, C.POINTER(C.c_float), _i32, _f32,
                                  _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp]),
    'ld_retina_targets_workspace_bytes': (_sz, [_G, _i32, _i32]),
    'ld_retina_targets': (C.c_int, [_G, _i32, _vp, _i32, _f32, _f32, _f32, _i32,
                                    _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_loss_prepass_ex': (C.c_int, [_G, _H, _M, _M, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _sz, _vp]),
    'ld_loss_prepass': (C.c_int, [_G, _H, _M, _M, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp, _sz, _vp]),
    'ld_loss_main': (C.c_int, [_G, _H, _M, _M, _M, _M, _M, _M, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _M, _M, _M,
                               _vp, _sz, _vp]),
    'ld_loss_main_parts': (C.c_int, [_G, _H, _M, _M, _M, _M, _M, _M, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _M, _M, _M, _M, _M, _M, _vp, _sz, _i32,
                                     _vp]),
    'ld_preprocess_batch': (C.c_int, [_vp, _i32, _i32, _i32,
                                      C.POINTER(C.c_float),
                                      C.POINTER(C.c_float), _i32, _vp, _vp]),
    'ld_preprocess_batch_aug': (C.c_int, [_vp, _i32, _i32, _i32,
                                          C.POINTER(C.c_float),
                                          C.POINTER(C.c_float),
                                          C.POINTER(C.c_float), _i32, _vp,
                                          _vp]),
    'ld_preprocess_batch_photo': (C.c_int, [_vp, _i32, _i32, _i32,
                                            C.POINTER(C.c_float),
                                            C.POINTER(C.c_float),
                                            C.POINTER(C.c_float), _i32, _vp,
                                            _vp]),
    'ld_jpeg_parse': (C.c_int, [_vp, _sz, C.POINTER(JpegInfoT)]),
    'ld_jpeg_entropy_decode': (C.c_int, [_vp, _sz, C.POINTER(JpegInfoT), _vp]),
    'ld_jpeg_entropy_decode_batch': (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32,
                                               _vp]),
    'ld_deform_im2col': (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32,
                                   _i32, _i32, _i32, _i32, _vp, _vp]),
    'ld_deform_offset_grad': (C.c_int, [_vp, _vp, _vp] + [_i32] * 9 +
                              [_vp, _vp]),
    'ld_deform_col2im_workspace_bytes': (_sz, [_i32] * 9),
    'ld_deform_col2im_index': (C.c_int, [_vp] + [_i32] * 9 + [_vp, _sz, _vp]),
    'ld_deform_col2im_sum': (C.c_int, [_vp] + [_i32] * 9 +
                             [_vp, _sz, _vp, _vp]),
    'ld_mdeform_im2col': (C.c_int, [_vp, _vp] + [_i32] * 9 + [_vp, _vp]),
    'ld_mdeform_offset_mask_grad': (C.c_int, [_vp, _vp, _vp] + [_i32] * 9 +
                                    [_vp, _vp]),
    'ld_mdeform_col2im_index': (C.c_int, [_vp] + [_i32] * 9 + [_vp, _sz, _vp]),
    'ld_quality_forward': (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp]),
    'ld_quality_backward_workspace_bytes': (_sz, [_i32, _i32]),
    'ld_quality_backward': (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _i32, _vp, _sz, _vp]),
    'ld_gi_region_workspace_bytes': (_sz, [_G]),
    'ld_gi_region': (C.c_int, [_G, _H, _M, _M, _M, _M, _i32, _f32, _vp, _vp,
                               _vp, _sz, _vp]),
    'ld_loss_finalize': (C.c_int, [_G, _H, _vp, _vp, _vp, _vp, _vp]),
    'ld_loss_centerness': (C.c_int, [_G, _H, _M, _vp, _vp, _vp, _vp, _M, _vp,
                                     _sz, _vp]),
    'ld_loss_set_reg_variant': (C.c_int, [_i32]),
    'ld_loss_plain_prepass': (C.c_int, [_G, _H, _D, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _sz, _vp]),
    'ld_loss_plain_pos': (C.c_int, [_G, _H, _D, _vp, _M, _M, _vp, _vp, _vp,
                                    _vp, _vp, _M, _vp, _sz, _vp]),
    'ld_l1_rows': (C.c_int, [_vp, _vp, _vp, _i64, _f32, _vp, _vp, _vp]),
    'ld_smooth_l1_rows': (C.c_int, [_vp, _vp, _vp, _i64, _f32, _f32, _vp, _vp,
                                    _vp]),
    'ld_delta_encode_rows': (C.c_int, [_D, _vp, _vp, _i64, _vp, _vp]),
    'ld_delta_decode_rows': (C.c_int, [_D, _vp, _vp, _i64,
                                       C.POINTER(C.c_float), _vp, _vp]),
    'ld_probe_copy': (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp]),
    'ld_probe_planes': (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    'ld_gconv_weight_image_floats': (_sz, [_i32, _i32, _i32, _i32]),
    'ld_gconv_weight_transform': (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp,
                                            _vp]),
    'ld_gconv_forward': (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32,
                                   _i32, _i32, _i32, _i32, _vp, _vp, _i32,
                                   _vp]),
    'ld_gconv_weight_image_bwd_floats': (_sz, [_i32, _i32, _i32, _i32]),
    'ld_gconv_weight_transform_bwd': (C.c_int, [_vp, _i32, _i32, _i32, _i32,
                                                _vp, _vp]),
    'ld_gconv_dgrad': (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                                 _i32, _i32, _i32, _i32, _i32, _vp]),
    'ld_gconv_wgrad_slabs': (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32]),
    'ld_gconv_wgrad_workspace_floats': (_sz, [_i32, _i32, _i32, _i32, _i32,
                                              _i32, _i32, _i32, _i32]),
    'ld_gconv_wgrad': (C.c_int, [_vp, _vp, _vp, _i32, _vp, _sz, _i32, _i32,
                                 _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                 _vp]),
    'ld_kl_integral_dense': (C.c_int, [_vp, _vp, _vp, _i64, _f32, _f32, _vp,
                                       _vp, _vp, _vp]),
    'ld_kd_kl_rows': (C.c_int, [_vp, _vp, _vp, _i64, _i32, _f32, _f32, _vp,
                                _vp, _vp]),
    'ld_qfl_rows': (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp,
                              _vp]),
    'ld_dfl_rows': (C.c_int, [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp,
                              _vp]),
    'ld_giou_rows': (C.c_int, [_vp, _vp, _vp, _i64, _f32, _f32, _vp, _vp,
                               _vp]),
    'ld_iou_rows': (C.c_int, [_vp, _vp, _vp, _i64, _f32, _i32, _f32, _vp, _vp,
                              _vp]),
    'ld_diou_rows': (C.c_int, [_vp, _vp, _vp, _i64, _f32, _f32, _vp, _vp,
                               _vp]),
    'ld_ciou_rows': (C.c_int, [_vp, _vp, _vp, _i64, _f32, _f32, _vp, _vp,
                               _vp]),
    'ld_integral_rows': (C.c_int, [_vp, _i64, _vp, _vp]),
    'ld_integral_rows_bwd': (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    'ld_bbox_overlaps': (C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _f32,
                                   _vp, _vp]),
    'ld_sum': (C.c_int, [_vp, _i64, _vp, _vp, _sz, _vp]),
    'ld_conv_weight_image_floats': (_sz, [_i32, _i32, _i32, _i32, _i32]),
    'ld_conv_weight_transform': (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp,
                                           _vp, _vp]),
    'ld_get_bboxes_workspace_bytes': (_sz, [_G, _i32, _i32]),
    'ld_get_bboxes': (C.c_int, [_G, _M, _M, _i32, _i32, _vp, _vp, _i32, _f32,
                                _f32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_get_bboxes_voting': (C.c_int, [_G, _M, _M, _i32, _i32, _vp, _vp, _i32, _f32,
                                _f32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_get_bboxes_num_selected': (C.c_int, [_G, _i32, _i32]),
    'ld_get_bboxes_pre_nms': (C.c_int, [_G, _M, _M, _M, _i32, _i32, _i32, _vp,
                                        _vp, _i32, _i32, _D, _vp, _vp, _vp, _vp,
                                        _vp, _sz, _vp]),
    'ld_get_bboxes_ex_workspace_bytes': (_sz, [_G, _i32, _i32, _i32]),
    'ld_get_bboxes_ex': (C.c_int, [_G, _M, _M, _M, _i32, _i32, _i32, _vp, _vp, _i32, _f32,
                                   _f32, _i32, _i32, _D, _vp, _vp, _vp, _vp, _vp,
                                   _sz, _vp]),
    'ld_aug_merge_nms_workspace_bytes': (_sz, [_AV, _i32, _i32]),
    'ld_aug_merge_nms': (C.c_int, [_AV, _i32, _i32, _f32, _f32, _i32, _i32,
                                   _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_eval_tpfp_workspace_bytes': (_sz, [_i32]),
    'ld_eval_tpfp': (C.c_int, [C.POINTER(EvalBatchT), _i32, _i32, _vp, _i32,
                               _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_eval_ap_workspace_bytes': (_sz, [_i32, _i32]),
    'ld_eval_ap': (C.c_int, [_i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32,
                             _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_eval_image_map_workspace_bytes': (_sz, [_i32, _i32]),
    'ld_eval_image_map': (C.c_int, [C.POINTER(EvalBatchT), _i32, _i32, _vp,
                                    _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_rank_images_workspace_bytes': (_sz, [_i32]),
    'ld_rank_images': (C.c_int, [_i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_draw_boxes': (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i32, _f32,
                                _i32, C.c_uint32, C.c_uint32, _vp]),
    'ld_draw_labels': (C.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _i32,
                                 C.c_uint32, C.c_uint32, _vp]),
    'ld_font_glyph': (C.c_int, [_i32, _i32]),
    'ld_eval_recalls_workspace_bytes': (_sz, [_i32, _i32, _i32, _i32]),
    'ld_eval_recalls_match': (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _i32,
                                        _i32, _i32, _i32, _vp, _i32, _vp,
                                        C.c_longlong, C.c_longlong, _vp, _sz,
                                        _vp]),
    'ld_eval_recalls_count': (C.c_int, [_vp, C.c_longlong, C.c_longlong, _i32,
                                        _i32, _vp, _vp, _vp]),
    'ld_coco_match_workspace_bytes': (_sz, [_i32, _i32, _i32, _i32]),
    'ld_coco_match': (C.c_int, [C.POINTER(CocoBatchT), _i32, _vp, _i32, _vp,
                                _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                _vp]),
    'ld_coco_match_errors_workspace_bytes': (_sz, [_i32, _i32, _i32, _i32]),
    'ld_coco_match_errors': (C.c_int, [C.POINTER(CocoErrBatchT), _i32, _vp,
                                       C.c_double, _i32, _vp, _i32, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_coco_accumulate_workspace_bytes': (_sz, [_i32, _i32, _i32, _i32,
                                                 _i32]),
    'ld_coco_accumulate': (C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _i32,
                                     _i32, _i32, _i32, _i32, _vp, _i32, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_conv_weight_transform_batch': (C.c_int, [_vp, _vp, _i32, _vp]),
    'ld_conv_weight_transform_tiles': (C.c_int, [_i32, _i32, _i32, _i32]),
    'ld_conv_weight_transform_batch_tiled': (C.c_int, [_vp, _vp, _i32, _i32,
                                                       _vp]),
    'ld_bn_prepare_batch': (C.c_int, [_vp, _vp, _i32, _vp]),
    'ld_conv_forward': (C.c_int, [_CV, _vp, _vp, _EP, _vp, _vp]),
    'ld_conv_forward_smallc': (C.c_int, [_CV, _vp, _vp, _EP, _vp, _vp]),
    'ld_conv_dgrad': (C.c_int, [_CV, _vp, _vp, _vp, _vp]),
    'ld_conv_dgrad_acc': (C.c_int, [_CV, _vp, _vp, _vp, _vp, _vp]),
    'ld_conv_tune_forward': (C.c_int, [_CV, _vp, _vp, _EP, _vp, _vp]),
    'ld_conv_tune_dgrad': (C.c_int, [_CV, _vp, _vp, _vp, _vp]),
    'ld_conv_bf16_weight_image_elems': (_sz, [_i32, _i32, _i32, _i32, _i32]),
    'ld_conv_bf16_weight_transform': (C.c_int, [_vp, _i32, _i32, _i32, _i32,
                                                _vp, _vp, _vp]),
    'ld_conv_bf16_weight_transform_batch': (C.c_int, [_vp, _vp, _i32, _vp]),
    'ld_conv_bf16_forward': (C.c_int, [_CV, _vp, _vp, _EP, _vp, _vp]),
    'ld_conv_bf16_tune_forward': (C.c_int, [_CV, _vp, _vp, _EP, _vp, _vp]),
    'ld_conv_bf16_dgrad': (C.c_int, [_CV, _vp, _vp, _vp, _vp]),
    'ld_conv_bf16_dgrad_acc': (C.c_int, [_CV, _vp, _vp, _vp, _vp, _vp]),
    'ld_conv_bf16_tune_dgrad': (C.c_int, [_CV, _vp, _vp, _vp, _vp]),
    'ld_conv_bf16_wgrad': (C.c_int, [_CV, _vp, _vp, _vp, _i32, _vp, _sz,
                                     _vp]),
    'ld_conv_bf16_wgrad_c8': (C.c_int, [_CV, _vp, _vp, _vp, _i32, _vp, _sz,
                                        _vp]),
    'ld_conv_to_c8': (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    'ld_conv_bf16_forward_c8': (C.c_int, [_CV, _vp, _vp, _EP, _vp, _vp]),
    'ld_conv_bf16_tune_forward_c8': (C.c_int, [_CV, _vp, _vp, _EP, _vp, _vp]),
    'ld_conv_bf16_dgrad_c8': (C.c_int, [_CV, _vp, _vp, _vp, _vp]),
    'ld_conv_bf16_dgrad_c8_acc': (C.c_int, [_CV, _vp, _vp, _vp, _vp, _vp]),
    'ld_record_begin': (C.c_int, []),
    'ld_record_end': (C.c_int64, []),
    'ld_record_abort': (C.c_int, []),
    'ld_record_count': (C.c_int, [C.c_int64]),
    'ld_record_replay': (C.c_int, [C.c_int64, _vp]),
    'ld_record_free': (C.c_int, [C.c_int64]),
    'ld_stream_fork': (C.c_int, [_vp, _vp]),
    'ld_step_list_build': (C.c_int64, [_vp, _i32]),
    'ld_copy_d2d': (C.c_int, [_vp, _vp, _sz, _vp]),
    'ld_step_list_info': (C.c_int, [C.c_int64, C.POINTER(C.c_int)]),
    'ld_step_list_replay': (C.c_int, [C.c_int64, _vp]),
    'ld_step_list_free': (C.c_int, [C.c_int64]),
    'ld_step_list_mark': (C.c_int, [_i32, _vp]),
    'ld_step_list_replay_until': (C.c_int, [C.c_int64, _vp, C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_void_p)]),
    'ld_step_list_last_failure': (C.c_int, [C.POINTER(C.c_int)]),
    'ld_bottleneck_c8_supported': (C.c_int, [_i32, _i32, _i32, _i32]),
    'ld_bottleneck_c8_forward': (C.c_int, [C.POINTER(BottleneckT), _vp, _vp,
                                           _vp]),
    'ld_conv_bf16_tune_dgrad_c8': (C.c_int, [_CV, _vp, _vp, _vp, _vp]),
    'ld_conv_tune_load': (C.c_int, [C.c_char_p]),
    'ld_conv_tune_save': (C.c_int, [C.c_char_p]),
    'ld_conv_tune_clear': (C.c_int, []),
    'ld_conv_tune_hits': (C.c_longlong, [C.POINTER(C.c_int32)]),
    'ld_conv_tune_reset_hits': (C.c_int, []),
    'ld_conv_wgrad_workspace_bytes': (_sz, [_CV]),
    'ld_conv_wgrad_partial': (C.c_int, [_CV, _i32, _vp, _vp, _vp, _sz,
                                        C.POINTER(WgradJobT), _vp]),
    'ld_wgrad_reduce_batch': (C.c_int, [_vp, _vp, _i32, _vp]),
    'ld_bn_act_backward_nsplit': (C.c_int, [_i32, _i32, _i32, _i32]),
    'ld_bias_grad_nsplit': (C.c_int, [_i32, _i32, _i32]),
    'ld_bias_grad_partial': (C.c_int, [_vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    'ld_bn_bwd_finalize_batch': (C.c_int, [_vp, _vp, _i32, _vp]),
    'ld_conv_tune_wgrad_workspace_bytes': (_sz, [_CV]),
    'ld_conv_wgrad': (C.c_int, [_CV, _vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    'ld_conv_tune_wgrad': (C.c_int, [_CV, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_conv_wgrad_plan': (C.c_int, [_CV, C.POINTER(C.c_int)]),
    'ld_conv_wgrad_smallc_supported': (C.c_int, [_CV]),
    'ld_conv_wgrad_smallc_slabs': (C.c_int, [_CV]),
    'ld_conv_wgrad_smallc_workspace_bytes': (_sz, [_CV]),
    'ld_conv_wgrad_smallc': (C.c_int, [_CV, _vp, _vp, _vp, _i32, _vp, _sz,
                                       _vp]),
    'ld_conv_wgrad_smallc_partial': (C.c_int, [_CV, _vp, _vp, _vp, _sz,
                                               C.POINTER(WgradJobT), _vp]),
    'ld_bn_prepare': (C.c_int, [_vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp,
                                _vp]),
    'ld_bn_act_forward_c8': (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                       _i32, _vp, _vp, _vp]),
    'ld_bn_act_forward': (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                    _i32, _vp, _vp]),
    'ld_bn_act_backward_workspace_bytes': (_sz, [_i32, _i32, _i32]),
    'ld_bn_act_backward': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32,
                                     _i32, _i32, _vp, _vp, _vp, _vp, _i32,
                                     _vp, _sz, _vp]),
    'ld_bn_act_backward_c8': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32,
                                        _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                        _vp, _i32, _vp, _sz, _vp]),
    'ld_bn_act_backward_c8in': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32,
                                          _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                          _vp, _i32, _vp, _sz, _vp]),
    'ld_bn_train_workspace_bytes': (_sz, [_i32, _i32, _i32]),
    'ld_bn_train_forward': (C.c_int, [_vp, _vp, _vp, _vp, _f32, C.c_double, _i32,
                                      _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_bn_train_backward': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32,
                                       _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp,
                                       _sz, _vp]),
    'ld_bias_grad': (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i32, _vp]),
    'ld_gn_forward_workspace_bytes': (_sz, [_LV, _i32, _i32]),
    'ld_gn_forward': (C.c_int, [_LV, _vp, _vp, _vp, _i32, _i32, _i32, _f32,
                                _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_gn_forward_c8': (C.c_int, [_LV, _vp, _vp, _vp, _i32, _i32, _i32, _f32,
                                   _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ld_gn_backward_c8': (C.c_int, [_LV, _vp, _vp, _vp, _vp, _vp, _vp, _i32,
                                    _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32,
                                    _vp, _sz, _vp]),
    'ld_gn_backward_c8_lean': (C.c_int, [_LV, _vp, _vp, _vp, _vp, _vp, _vp, _i32,
                                         _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32,
                                         _vp, _sz, _vp]),
    'ld_gn_backward_workspace_bytes': (_sz, [_LV, _i32, _i32]),
    'ld_gn_backward': (C.c_int, [_LV, _vp, _vp, _vp, _vp, _vp, _vp, _i32,
                                 _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp,
                                 _sz, _vp]),
    'ld_maxpool3x3s2': (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    'ld_maxpool_3x3s2_backward': (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp,
                                           _vp]),
    'ld_res2_gather': (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32,
                                 C.c_longlong, _vp, _vp]),
    'ld_res2_concat': (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                                 _i32, _i32, _i32, _i32, _vp, _vp]),
    'ld_avgpool_ceil_forward': (C.c_int, [_vp, C.c_longlong, _i32, _i32, _i32,
                                          _vp, _vp]),
    'ld_avgpool_ceil_backward': (C.c_int, [_vp, C.c_longlong, _i32, _i32,
                                           _i32, _vp, _vp]),
    'ld_upsample_add_forward': (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32,
                                          _i32, _vp, _vp]),
    'ld_upsample_add_backward': (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32,
                                           _vp, _vp]),
    'ld_upsample_add_backward_acc': (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32,
                                               _vp, _vp, _vp]),
    'ld_pack_levels': (C.c_int, [_LV, C.POINTER(C.c_void_p), _i32, _vp, _vp]),
    'ld_unpack_levels': (C.c_int, [_LV, _vp, _i32, C.POINTER(C.c_void_p), _vp]),
    'ld_pack_levels_c8': (C.c_int, [_LV, C.POINTER(C.c_void_p), _i32, _i32, _vp,
                                    _vp, _vp]),
    'ld_unpack_levels_c8': (C.c_int, [_LV, _vp, _i32, _i32,
                                      C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), _vp]),
    'ld_scale_levels_forward': (C.c_int, [_LV, _vp, _vp, _i32, _vp, _vp]),
    'ld_scale_levels_backward_workspace_bytes': (_sz, [_LV]),
    'ld_scale_levels_backward': (C.c_int, [_LV, _vp, _vp, _vp, _i32, _vp, _vp,
                                           _i32, _vp, _sz, _vp]),
    'ld_scale_act_levels_forward': (C.c_int, [_LV, _vp, _vp,
                                              C.POINTER(C.c_int32), _i32, _i32,
                                              _vp, _vp]),
    'ld_scale_act_levels_backward': (C.c_int, [_LV, _vp, _vp, _vp, _vp,
                                               C.POINTER(C.c_int32), _i32,
                                               _i32, _vp, _vp, _i32, _vp, _sz,
                                               _vp]),
    'ld_sgd_step': (C.c_int, [_vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32,
                              _vp]),
    'ld_sgd_step_dev': (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    'ld_sgd_step_classes': (C.c_int, [_vp, _vp, _vp, _sz, _vp, _i32, _vp, _vp,
                                      _vp]),
    'ld_grad_norm_workspace_bytes': (_sz, []),
    'ld_grad_norm': (C.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    'ld_vrank_reduce': (C.c_int, [_vp, _i32, _i32, _sz, _vp, _vp]),
    'ld_levels_mix': (C.c_int, [_vp, _vp, C.c_longlong, _i32, _vp, _vp, _vp]),
    'ld_levels_abs_err_workspace_bytes': (_sz, [_LV, _i32, _i32, _i32]),
    'ld_levels_abs_err': (C.c_int, [_LV, _vp, _vp, _i32, _i32, _i32, _vp, _vp,
                                    _sz, _vp]),
    'ld_levels_pearson_workspace_bytes': (_sz, [_LV, _i32, _i32, _i32]),
    'ld_levels_pearson': (C.c_int, [_LV, _vp, _vp, _i32, _i32, _i32, _vp, _vp,
                                    _vp, _sz, _vp]),
}


def _declare(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


_ERR = {-1: 'LD_EINVAL (bad argument)', -2: 'LD_ENOSPACE (workspace too small)',
        -3: 'LD_EUNSUPPORTED'}


def check(rc, what):
    if rc != 0:
        raise LdError(f'{what} failed: {_ERR.get(rc, "hipError_t %d" % rc)}')


# ---------------------------------------------------------------------------
# tensor plumbing
# ---------------------------------------------------------------------------
def require_device(t, dtype=None, name='tensor'):
    """The product runs on the GPU only: refuse anything else, loudly."""
    if not isinstance(t, torch.Tensor):
        raise LdError(f'{name}: expected a torch.Tensor, got {type(t)}')
    if not t.is_cuda:
        raise LdError(
            f'{name} is on {t.device}: ld_amd ops only run on a HIP device '
            '(there is no CPU path)')
    if dtype is not None and t.dtype != dtype:
        raise LdError(f'{name}: expected {dtype}, got {t.dtype}')
    return t


# While a launch list is being recorded (ld_record_begin .. ld_record_end, see
# detectors.TeacherPlan) every tensor whose address goes to the library is kept
# alive with the list: a replay re-issues the launches with these very pointers.
_KEEP = [None]


def ptr(t):
    if t is None:
        return C.c_void_p(0)
    k = _KEEP[0]
    if k is not None:
        k.append(t)
    return C.c_void_p(t.data_ptr())


def keep(*ts):
    """For call sites that put ``t.data_ptr()`` into a struct themselves."""
    k = _KEEP[0]
    if k is not None:
        k.extend(t for t in ts if t is not None)


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_ptr(device=None):
    """The current HIP stream of ``device`` as a void*.  (torch.cuda.
    current_stream() builds a Python Stream object per call: 4-5 us, ~420 calls
    per step in the round-5 host profile; the raw accessor is a plain C call.)"""
    if isinstance(device, torch.device) and device.type != 'cuda':
        return C.c_void_p(0)
    if _RAW_STREAM is not None:
        if device is None:
            idx = torch.cuda.current_device()
        elif isinstance(device, int):
            idx = device
        else:
            idx = device.index
            if idx is None:
                idx = torch.cuda.current_device()
        return C.c_void_p(_RAW_STREAM(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def stream_id(device=None):
    """An integer identifying the current stream (cache keys)."""
    return stream_ptr(device).value or 0


def make_geom(featmap_sizes, strides, num_imgs, anchor_scale=8):
    g = GeomT()
    L = len(featmap_sizes)
    if L > LD_MAX_LEVELS or L != len(strides):
        raise LdError('bad pyramid geometry')
    off = 0
    for l, ((h, w), s) in enumerate(zip(featmap_sizes, strides)):
        s = s[0] if isinstance(s, (tuple, list)) else s
        g.lv[l].H, g.lv[l].W = int(h), int(w)
        g.lv[l].stride, g.lv[l].offset = int(s), off
        off += int(h) * int(w)
    g.num_levels, g.num_anchors = L, off
    g.num_imgs, g.anchor_scale = int(num_imgs), int(anchor_scale)
    return g


def make_maps(tensors):
    """Per-level (N, C, H, W) fp32 device tensors -> MapsT.  Each tensor's
    spatial block must be contiguous (stride (.., .., W, 1)); batch and
    channel strides are free, so views into a level-concatenated (N, C, A)
    arena work without copies."""
    m = MapsT()
    for l, t in enumerate(tensors):
        require_device(t, torch.float32, f'level {l} map')
        n, c, h, w = t.shape
        sn, sc, sh, sw = t.stride()
        if (w > 1 and sw != 1) or (h > 1 and sh != w):
            raise LdError(f'level {l} map: spatial block is not contiguous')
        m.ptr[l] = t.data_ptr()
        m.stride_n[l] = sn
        m.stride_c[l] = sc
    return m
