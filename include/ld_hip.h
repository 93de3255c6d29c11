/* ld_hip.h -- C ABI of libldhip.so, the MI355X (gfx950) implementation of the
 * HikariTJU/LD training hot path.
 *
 * The reference (an MMDetection 2.10 fork, pure Python) has no native
 * boundary of its own: its drop-in boundary is the mmdet registry API
 * (SURVEY.md section 8b).  The host-side mirror of that API lives in the
 * Python package `ld_amd`; every arithmetic step underneath it goes through
 * the entry points declared here.  Each entry point cites the reference
 * function it replaces (file:line relative to the reference checkout).
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers unless the
 *    parameter is a `const ld_*_t*` descriptor struct (host memory, read
 *    during the call) or says "host";
 *  - no allocation, no synchronisation and no host read-back inside: callers
 *    pass workspaces; every launch goes to `stream` (a hipStream_t);
 *  - return 0 on success, a negative LD_E* code on a bad argument, or the
 *    positive hipError_t of a failed launch.  Nothing throws.
 *  - tensors are fp32 unless stated; label tensors are int64 as in the
 *    reference (ld_head.py:522-530).
 */
#ifndef LD_HIP_H_
#define LD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LD_MAX_LEVELS 8
#define LD_NUM_LOSS_KEYS 8 /* loss_cls,bbox,dfl,ld,ld_vlr,kd,kd_neg,im */

#define LD_EINVAL (-1)   /* bad argument */
#define LD_ENOSPACE (-2) /* workspace too small */
#define LD_EUNSUPPORTED (-3)

typedef void* ld_stream_t; /* hipStream_t */

/* ---- geometry of the FPN pyramid ------------------------------------- */
/* One anchor per feature-map cell, anchors ordered level-major then row-major
 * (x fastest): anchor_generator.py:229-270, ld_head.py:396-403. */
typedef struct {
  int32_t H, W;     /* feature-map size of this level            */
  int32_t stride;   /* anchor stride (8,16,32,64,128)            */
  int32_t offset;   /* index of the level's first anchor         */
} ld_level_t;

typedef struct {
  int32_t num_levels;
  int32_t num_anchors;      /* sum of H*W over levels                */
  int32_t num_imgs;         /* N                                     */
  int32_t anchor_scale;     /* octave_base_scale (8): side = scale*stride */
  ld_level_t lv[LD_MAX_LEVELS];
} ld_geom_t;

/* A per-level family of NCHW maps (N, C, H_l, W_l).  Element (n, c, y, x) of
 * level l lives at ptr[l] + n*stride_n[l] + c*stride_c[l] + y*W_l + x, which
 * covers both separately allocated level tensors and the level-concatenated
 * (N, C, A) arena the head uses. */
typedef struct {
  float* ptr[LD_MAX_LEVELS];
  int64_t stride_n[LD_MAX_LEVELS];
  int64_t stride_c[LD_MAX_LEVELS];
} ld_maps_t;

/* Hyper-parameters of LDHead.loss (ld_head.py:47-71 and the loss modules'
 * constructor arguments). */
typedef struct {
  int32_t num_classes; /* 80 */
  int32_t reg_max;     /* 16 -> 17 bins; only 16 is compiled */
  int32_t topk;        /* ATSS topk, 9 */
  int32_t feat_channels; /* 256 (ld_head.py:153-154 hard-codes it) */
  float lw_cls, qfl_beta;       /* QualityFocalLoss (beta must be 2) */
  float lw_bbox, giou_eps;      /* GIoULoss / IoULoss / DIoULoss / CIoULoss: eps */
  float lw_dfl;                 /* DistributionFocalLoss */
  float lw_ld, T_ld;            /* KnowledgeDistillationKLDivLoss (main LD) */
  float lw_ld_vlr, T_ld_vlr;    /* ... (VLR LD)    */
  float lw_kd, T_kd;            /* ... (cls KD)    */
  float lw_im;                  /* IMLoss          */
  /* GFLv2 / LDv2 (gfocal_head.py:201-217, ld_gflv2.py:116-282): the class
   * map is cls_score = sigmoid(cls_feat) * quality, a PROBABILITY with
   * cls_channels = num_classes + 1 channels (use_sigmoid=False,
   * anchor_head.py:68-71).  With LD_LOSS_PROB_CLS: QFL uses
   * binary_cross_entropy on probabilities (gfocal_loss.py:27-30),
   * weight_targets = max_c cls_score without a sigmoid (ld_gflv2.py:200) and
   * the KD term runs on the separate kd_* maps (raw cls_feat, ld_gflv2.py:243).
   * cls_channels = 0 means num_classes. */
  int32_t cls_channels;
  int32_t flags;
  /* LD_LOSS_ATSS (LDATSSHead over ATSSGFLHead, ld_atss.py:44-250): loss_cls is
   * the sigmoid FocalLoss (gamma = qfl_beta = 2, focal_alpha) instead of QFL;
   * the GIoU term is weighted by the ATSS centerness target and normalised by
   * the sum of those targets (1 if that sum is < 1e-12); a centerness BCE term
   * (lw_ctr, ld_loss_centerness) is added and reported in the loss_kd_neg row;
   * there is no DFL term (set lw_dfl = 0) and loss_ld_neg = 0.15 * loss_ld's
   * module on the VLR region (set lw_ld_vlr = 0.6 * lw_ld, T_ld_vlr = T_ld). */
  float lw_ctr, focal_alpha;
} ld_loss_hp_t;
#define LD_LOSS_PROB_CLS 1
/* target assignment: the imitation region is "anchor centre strictly inside a
 * GT box" (get_im_region modes 'fitnet' / 'decouple' / 'gibox',
 * ld_head.py:597-611) instead of the 'finegrained' IoU rule (:594-596) */
#define LD_IM_CENTER_INSIDE 2
#define LD_LOSS_ATSS 4
/* with LD_LOSS_ATSS: LDFCOSHead over FCOSGFLHead (ld_fcos_head.py:46-217).
 * Points instead of anchors: the cell centre is (x + 0.5, y + 0.5) strides,
 * bbox_targets hold (left, top, right, bottom) distances in pixels
 * (ld_fcos_targets), the centerness target comes from those distances, and the
 * VLR term is weighted by vlr * max_c sigmoid(cls) (the "remain" points,
 * ld_fcos_head.py:117-131; set lw_ld_vlr = lw_ld for its 0.25 factor). */
#define LD_LOSS_FCOS 8
/* LDRetinaHead over RetinaGFLHead (ld_retina.py:41-137), B anchors per cell:
 * the caller views its (N, B * C, H, W) maps as (N * B, C, H, W) -- N * B
 * pseudo-images with one anchor per cell -- and passes geom.num_imgs = N * B
 * with the target arrays of ld_retina_targets.  FocalLoss (focal_alpha) on
 * every anchor with label_weights (0 in the ignore band); GIoU with weight 1
 * on the positives; loss_cls and loss_bbox divided by num_total_pos
 * (counts[num_imgs + 2L], LOCAL: the head takes no cross-rank mean); LD and
 * the VLR term take the softmax over ALL 68 corner logits of an anchor (the
 * head hands (rows, 68) to the KL loss, ld_retina.py:87-110), weights max_c
 * sigmoid(cls) on the positives / the VLR value on background anchors, both
 * with avg_factor 4 (set lw_ld_vlr = 0.03 * 4 * lw_ld, T_ld_vlr = T_ld); no DFL
 * (lw_dfl = 0); KD on the positives' class logits as in LDHead. */
#define LD_LOSS_RETINA 16
/* The box loss loss_pos_kernel evaluates on the decoded positives, uniform per
 * launch: a 3-bit field at LD_LOSS_BBOX_SHIFT.  0 = GIoULoss, so a flags word
 * without the field means what it always meant.  giou_eps carries the
 * module's eps for all of them (iou_loss.py:14-36,85-219). */
#define LD_LOSS_BBOX_SHIFT 8
#define LD_LOSS_BBOX_MASK 7
#define LD_LOSS_BBOX_GIOU 0
#define LD_LOSS_BBOX_IOU 1        /* IoULoss(linear=False): -log IoU */
#define LD_LOSS_BBOX_IOU_LINEAR 2 /* IoULoss(linear=True): 1 - IoU */
#define LD_LOSS_BBOX_DIOU 3
#define LD_LOSS_BBOX_CIOU 4
/* Plain ATSSHead / RetinaHead (atss_head.py:145-296, anchor_head.py:376-495):
 * the reg maps carry the 4 DeltaXYWH deltas of an anchor instead of 68
 * distribution logits.  Combined with LD_LOSS_ATSS or LD_LOSS_RETINA (which keep
 * their class, centerness and normaliser rules); the block is then run as
 * ld_loss_plain_prepass -> ld_loss_plain_pos -> ld_loss_main_parts(
 * LD_LOSS_PART_CLS) [-> ld_loss_centerness] -> ld_loss_finalize: no REG / IM
 * launch, no teacher maps, the DFL, LD, VLR-LD, KD and IM rows of the table are
 * zero (set lw_kd = 0).  The coder travels beside hp in an ld_delta_t. */
#define LD_LOSS_DELTA 32
/* Plain FCOSHead (fcos_head.py:157-254): with LD_LOSS_ATSS | LD_LOSS_FCOS (which
 * keep the FocalLoss, the centerness BCE, the point geometry and the (l, t, r, b)
 * targets of ld_fcos_targets), never with LD_LOSS_DELTA, LD_LOSS_RETINA or
 * LD_LOSS_PROB_CLS.  The reg maps carry 4 ACTIVATED distances per point
 * (ld_scale_act_levels_forward: exp or relu of the scaled conv output).  The
 * block runs as ld_loss_plain_prepass -> ld_loss_plain_pos -> ld_loss_main_parts(
 * LD_LOSS_PART_CLS) -> ld_loss_centerness -> ld_loss_finalize; the DFL, LD,
 * VLR-LD, KD and IM rows are zero.  loss_cls and loss_centerness are divided by
 * max(num_pos, 1), loss_bbox by max(sum of the centerness targets, 1e-6).
 * LD_LOSS_DIST_NORM (only with LD_LOSS_DIST) = norm_on_bbox: the targets are
 * divided by the level's stride and compared with the prediction as it is, about
 * the pixel points (fcos_head.py:233-236, 524-525). */
#define LD_LOSS_DIST 64
#define LD_LOSS_DIST_NORM 128

/* DeltaXYWHBBoxCoder (delta_xywh_bbox_coder.py:26-237) and what the box term of
 * an LD_LOSS_DELTA block does with it. */
typedef struct {
  float means[4], stds[4]; /* target_means, target_stds */
  float max_ratio;         /* |log(wh_ratio_clip)|: the clamp of dw, dh in decode */
  float beta;              /* SmoothL1Loss beta (LD_DELTA_SMOOTH_L1) */
  int32_t num_base;        /* anchors per cell of the explicit anchor list; 0 = the
                              implicit square anchor of side anchor_scale * stride */
  int32_t box_term;        /* LD_DELTA_* below */
} ld_delta_t;
/* the box loss of the positives:
 *   DECODED    hp's LD_LOSS_BBOX_* loss on delta2bbox(anchor, pred) against the
 *              target box (LD_LOSS_ATSS: the target encoded and decoded again,
 *              atss_head.py:193-205; LD_LOSS_RETINA: reg_decoded_bbox=True,
 *              anchor_head.py:414-424)
 *   L1 / SMOOTH_L1  on pred - bbox2delta(anchor, gt), summed over the four
 *              deltas (reg_decoded_bbox=False; LD_LOSS_RETINA only) */
#define LD_DELTA_DECODED 0
#define LD_DELTA_L1 1
#define LD_DELTA_SMOOTH_L1 2

/* ---- library ------------------------------------------------------------ */
/* ABI version of this header; bump on any signature change. */
int ld_abi_version(void);
/* Name of the gfx target the kernels were compiled for ("gfx950"). */
const char* ld_target_arch(void);

/* ---- target assignment ---------------------------------------------------
 * Replaces, for a whole batch in two launches:
 *   AnchorHead.get_anchors            anchor_head.py:145-173 (anchors implicit)
 *   anchor_inside_flags               core/anchor/utils.py:20-46
 *   ATSSAssigner.assign               atss_assigner.py:33-181
 *   PseudoSampler.sample              samplers/pseudo_sampler.py:24-41
 *   ATSSAssigner.get_vlr_region       atss_assigner.py:183-298
 *   LDHead.get_im_region('finegrained') ld_head.py:580-611
 *   LDHead._get_target_single/unmap   ld_head.py:449-577
 *
 * gt_bboxes  (N, max_gt, 4) xyxy, rows >= num_gt[n] ignored
 * gt_labels  (N, max_gt) int64
 * num_gt     (N) int32
 * valid_hw   (N, num_levels, 2) int32: valid_h, valid_w of each level from
 *            img_meta['pad_shape'] (anchor_generator.py:293-300)
 * outputs, dense (N, A): labels int64 (background = num_classes),
 *   label_weights, bbox_targets (N, A, 4), vlr, im
 * counts     int32 [N + 2*num_levels + 1]:
 *            [0,N) positives per image; [N, N+L) positives per level (batch);
 *            [N+L, N+2L) im-region anchors per level; [N+2L] = sum_i max(P_i,1)
 * Tie rule: equal centre distances are ordered by lower anchor index (the
 * reference's order is an artefact of torch.topk). */
size_t ld_atss_targets_workspace_bytes(const ld_geom_t* geom, int max_gt);
int ld_atss_targets(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                    const float* gt_bboxes, const int64_t* gt_labels,
                    const int32_t* num_gt, int max_gt, const int32_t* valid_hw,
                    int64_t* labels, float* label_weights, float* bbox_targets,
                    float* vlr, float* im, int32_t* counts, void* workspace,
                    size_t workspace_bytes, ld_stream_t stream);

/* Same, with (a) optional EXPLICIT anchors (A, 4) -- the reference-style
 * ATSSAssigner.assign(bboxes, num_level_bboxes, ...) entry, where a level is
 * just an index range: pass geometry levels with H = count, W = 1 -- and
 * (b) optional per-anchor assign results: gt_inds (N, A) int64 1-based / 0,
 * max_overlaps (N, A) (-1e8 where unassigned) as AssignResult carries them
 * (atss_assigner.py:163-181).  anchors / gt_inds / max_overlaps may be NULL. */
int ld_atss_targets_ex(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                       const float* anchors, const float* gt_bboxes,
                       const int64_t* gt_labels, const int32_t* num_gt,
                       int max_gt, const int32_t* valid_hw, int64_t* labels,
                       float* label_weights, float* bbox_targets, float* vlr,
                       float* im, int32_t* counts, int64_t* gt_inds,
                       float* max_overlaps, void* workspace,
                       size_t workspace_bytes, ld_stream_t stream);

/* Materialise the anchors (A, 4) -- only for API compatibility
 * (AnchorGenerator.grid_anchors, anchor_generator.py:207-270); the kernels
 * never read them. */
/* FCOS point targets for the whole batch (LDFCOSHead.get_targets,
 * ld_fcos_head.py:261-414): same output arrays as ld_atss_targets; bbox_targets
 * = (l, t, r, b) distances of the assigned object, vlr = 1 on the points that
 * lie inside some gt box but are assigned to none ("remain"), label_weights = 1,
 * im = 0.  regress_ranges: HOST float[2 * num_levels] (lo, hi per level).
 * counts[N + 2L] = total number of positives (no per-image floor). */
int ld_fcos_targets(const ld_geom_t* geom, int num_classes,
                    const float* regress_ranges, int center_sampling,
                    float center_sample_radius, const float* gt_bboxes,
                    const int64_t* gt_labels, const int32_t* num_gt, int max_gt,
                    int64_t* labels, float* label_weights, float* bbox_targets,
                    float* vlr, float* im, int32_t* counts, ld_stream_t stream);
int ld_grid_anchors(const ld_geom_t* geom, float* anchors, ld_stream_t stream);

/* MaxIoU targets for a head with ``num_base`` anchors per cell
 * (LDRetinaHead.get_targets / _get_targets_single, ld_retina.py:256-470):
 * MaxIoUAssigner.assign (max_iou_assigner.py:93-212; match_low_quality and
 * gt_max_assign_all on, no ignore boxes, float neg_iou_thr) + PseudoSampler +
 * the head's get_vlr_region (ld_retina.py:478-603).  ``geom`` describes the N
 * real images and the H x W cells; ``anchors`` is the explicit list
 * (num_anchors * num_base, 4) in AnchorGenerator.grid_anchors order (level,
 * cell, base anchor fastest).  Outputs use the PSEUDO-IMAGE layout
 * [(n * num_base + b) * num_anchors + cell] (see LD_LOSS_RETINA): labels
 * (background = num_classes), label_weights (1 on positives and negatives, 0 in
 * the band between the thresholds and outside the valid region), bbox_targets
 * (the matched gt box, xyxy pixels), vlr, im (zeros), optional gt_inds (-1
 * ignored / 0 negative / g + 1).  counts: int32[N * num_base + 2L + 1]: positives
 * per pseudo-image, per level, (unused), and at [N * num_base + 2L] the
 * reference's num_total_pos = sum over REAL images of max(P_i, 1). */
size_t ld_retina_targets_workspace_bytes(const ld_geom_t* geom, int num_base,
                                         int max_gt);
int ld_retina_targets(const ld_geom_t* geom, int num_base, const float* anchors,
                      int num_classes, float pos_iou_thr, float neg_iou_thr,
                      float min_pos_iou, int topk, const float* gt_bboxes,
                      const int64_t* gt_labels, const int32_t* num_gt, int max_gt,
                      const int32_t* valid_hw, int64_t* labels,
                      float* label_weights, float* bbox_targets, float* vlr,
                      float* im, int32_t* counts, int64_t* gt_inds,
                      void* workspace, size_t workspace_bytes, ld_stream_t stream);

/* ---- fused loss block ----------------------------------------------------
 * Replaces LDHead.loss_single for all levels and images, forward AND gradient
 * (ld_head.py:116-282), reading the head outputs NCHW-direct (no permute).
 *
 * Call order on one stream:
 *   ld_loss_prepass   -> weight_targets, IoU score, partial normalisers
 *   (optional cross-rank all-reduce of norm_partial[0..1])
 *   ld_loss_main      -> loss partials + gradients
 *   ld_loss_finalize  -> the (8, L) loss table
 *
 * norm (device, float[4]): [0] sum_i max(P_i,1) (this rank), [1] sum of
 *   weight_targets (this rank); after the caller's optional mean over ranks
 *   ld_loss_main reads NTS = max(norm[0],1) and AVG = norm[1] + 1e-6 from it
 *   (ld_head.py:338-341,362-365).
 */
size_t ld_loss_workspace_bytes(const ld_geom_t* geom);

/* weight_targets = max_c sigmoid(cls) at positives (ld_head.py:198-199),
 * score = IoU(decoded box, target) (ld_head.py:200-207) written dense (N, A)
 * (zero elsewhere); norm[0], norm[1] as above. */
int ld_loss_prepass(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                    const ld_maps_t* cls, const ld_maps_t* reg,
                    const int64_t* labels, const float* bbox_targets,
                    const int32_t* counts, float* weight_targets, float* score,
                    float* norm, void* workspace, size_t workspace_bytes,
                    ld_stream_t stream);

/* The same with the VLR array: needed by LD_LOSS_FCOS (weight_targets are also
 * produced where vlr > 0); vlr may be NULL otherwise. */
int ld_loss_prepass_ex(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                       const ld_maps_t* cls, const ld_maps_t* reg,
                       const int64_t* labels, const float* bbox_targets,
                       const float* vlr, const int32_t* counts,
                       float* weight_targets, float* score, float* norm,
                       void* workspace, size_t workspace_bytes, ld_stream_t stream);

/* Forward + gradient of every loss term.  grad_* have the same descriptors
 * as their inputs and are fully overwritten.  `upstream` (device,
 * float[8 * num_levels] key-major like `losses`, may be NULL = all ones) is
 * d total / d loss[key][level] (base.py:197-210 sums them, so it is 1). */
int ld_loss_main(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                 const ld_maps_t* cls, const ld_maps_t* reg,
                 const ld_maps_t* t_cls, const ld_maps_t* t_reg,
                 const ld_maps_t* x, const ld_maps_t* t_x,
                 const int64_t* labels, const float* label_weights,
                 const float* bbox_targets, const float* vlr, const float* im,
                 const int32_t* counts, const float* weight_targets,
                 const float* score, const float* norm, const float* upstream,
                 const ld_maps_t* grad_cls, const ld_maps_t* grad_reg,
                 const ld_maps_t* grad_x, void* workspace,
                 size_t workspace_bytes, ld_stream_t stream);

/* The same with a launch mask: ld_loss_main runs four dense launches --
 * POS (the positive anchors: GIoU + class-softmax statistics), REG (thread =
 * anchor x side: LD-KL + VLR-LD + DFL + the GIoU chain through Integral,
 * forward and gradient -- the north-star fused LD-KL + Integral sweep), CLS
 * (anchor x 16 classes: QFL + KD), IM (anchor x 32 channels: masked MSE).
 * `parts` selects which of them run (benchmarking one kernel of the step at a
 * saturating size; REG/CLS read what POS wrote for the positive anchors).
 * kd_s / kd_t / grad_kd: student / teacher maps of the KD term and its
 * gradient map when they are not the class maps themselves (LDv2: raw
 * cls_feat); NULL = cls / t_cls / grad_cls (LDHead: KD adds into grad_cls). */
#define LD_LOSS_PART_POS 1
#define LD_LOSS_PART_REG 2
#define LD_LOSS_PART_CLS 4
#define LD_LOSS_PART_IM 8
#define LD_LOSS_PART_ALL 15
/* Selects the kernel the REG part launches (benchmarking / A-B tests; the
 * default is the measured best, profiles/r03_ldkl_variants.json).  variant:
 * bits 0-1 log2(anchors per thread: 1, 2, 4) | bit 2 non-temporal loads | bit 3
 * non-temporal stores | bit 4 hardware exp / rcp | bit 5 the four sides of an
 * anchor chunk in adjacent workgroups | bit 6 the NT bits also apply to maps
 * that fit the Infinity Cache | bit 7 (1 anchor per thread only) hold the
 * kernel to 64 VGPRs = 8 waves per SIMD | bit 16 (with bit 5) those four
 * workgroups on one XCD | bits 8-15 KiB of dynamic LDS per workgroup
 * (occupancy throttle); < 0 = the round-2 kernel (which LD_LOSS_RETINA and
 * T_ld != T_ld_vlr always use).  Returns the previous value (-1 if it was
 * negative), LD_EINVAL on a malformed word.  Not thread-safe; set it between
 * launches. */
int ld_loss_set_reg_variant(int variant);
/* LD_LOSS_ATSS only: the centerness term.  ctr / grad_ctr: (N, 1, H_l, W_l)
 * maps; score = the centerness targets ld_loss_prepass wrote; call between
 * ld_loss_main_parts and ld_loss_finalize (same workspace). */
int ld_loss_centerness(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                       const ld_maps_t* ctr, const int64_t* labels,
                       const float* score, const float* norm, const float* upstream,
                       const ld_maps_t* grad_ctr, void* workspace,
                       size_t workspace_bytes, ld_stream_t stream);
int ld_loss_main_parts(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                       const ld_maps_t* cls, const ld_maps_t* reg,
                       const ld_maps_t* t_cls, const ld_maps_t* t_reg,
                       const ld_maps_t* x, const ld_maps_t* t_x,
                       const int64_t* labels, const float* label_weights,
                       const float* bbox_targets, const float* vlr, const float* im,
                       const int32_t* counts, const float* weight_targets,
                       const float* score, const float* norm, const float* upstream,
                       const ld_maps_t* grad_cls, const ld_maps_t* grad_reg,
                       const ld_maps_t* grad_x, const ld_maps_t* kd_s,
                       const ld_maps_t* kd_t, const ld_maps_t* grad_kd,
                       void* workspace, size_t workspace_bytes, int parts,
                       ld_stream_t stream);

/* The two launches a plain block (LD_LOSS_DELTA or LD_LOSS_DIST, never both)
 * has of its own.  `delta` selects the form: non-NULL exactly with
 * LD_LOSS_DELTA, NULL exactly with LD_LOSS_DIST; any other pairing, and any flag
 * combination but the ones those two flags name, is LD_EINVAL.
 * reg / grad_reg: (N, 4, H_l, W_l) maps.  Same workspace as the other parts.
 *
 * LD_LOSS_DELTA (with exactly one of LD_LOSS_ATSS / LD_LOSS_RETINA): reg holds
 * DeltaXYWH deltas (LD_LOSS_RETINA: the (N * B, 4, ...) pseudo-image views).
 * anchors: the explicit (num_anchors * num_base, 4) list, row (cell * num_base +
 * b), when delta->num_base > 0 (pseudo-image n uses base anchor n % num_base, so
 * num_imgs is a multiple of num_base); NULL for the implicit square anchor.
 * bbox_targets hold the matched GT boxes in pixels, as the target launches write
 * them.
 * LD_LOSS_DIST: reg holds activated distances, anchors is NULL; bbox_targets:
 * ld_fcos_targets' (l, t, r, b) in pixels.
 *
 * prepass: score = the centerness target sqrt(min(l, r) / max(l, r) * min(t, b) /
 * max(t, b)) of the positives -- delta: from the anchor centre and the
 * encoded-then-decoded GT (atss_head.py:298-313; zero with LD_LOSS_RETINA);
 * dist: of the targets themselves --, weight_targets = 0, norm as
 * ld_loss_prepass leaves it (num_pos, sum of the centerness targets).
 * pos: the box term, forward and gradient, written dense into grad_reg (zeros
 * away from the positives), and the class-softmax statistics
 * ld_loss_main_parts(CLS) reads.  delta: through the decode -- the gradient of a
 * clamped dw / dh is zero.  dist: hp's LD_LOSS_BBOX_* loss on (px - d0, py - d1,
 * px + d2, py + d3) against the same form of the targets, (px, py) = (x, y) *
 * stride + stride / 2, weighted by the centerness target; d(loss)/d(d) =
 * (-g.x1, -g.y1, +g.x2, +g.y2). */
int ld_loss_plain_prepass(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                          const ld_delta_t* delta, const float* anchors,
                          const int64_t* labels, const float* bbox_targets,
                          const int32_t* counts, float* weight_targets, float* score,
                          float* norm, void* workspace, size_t workspace_bytes,
                          ld_stream_t stream);
int ld_loss_plain_pos(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                      const ld_delta_t* delta, const float* anchors,
                      const ld_maps_t* cls, const ld_maps_t* reg,
                      const int64_t* labels, const float* bbox_targets,
                      const float* score, const float* norm, const float* upstream,
                      const ld_maps_t* grad_reg, void* workspace,
                      size_t workspace_bytes, ld_stream_t stream);

/* The 'gibox' imitation region (LDHead.get_gi_region, ld_head.py:613-637;
 * LDv2Head: ld_gflv2.py:619-644 with hp->flags & LD_LOSS_PROB_CLS): per level,
 * over all cells of all images, the General-Instance score max_c |teacher -
 * student| and box (the winner's decoded distribution), then the first `topn`
 * (10) survivors of a greedy NMS at `iou_thr` (0.3) -- torchvision.ops.nms's
 * published semantics: descending score, IoU > thr suppresses.  Writes the
 * (N, A) 0/1 mask `im` and the per-level selected counts into
 * counts[N + L + l] (the slots ld_loss_main reads for loss_im); run it between
 * ld_atss_targets and ld_loss_main.  Equal scores: lower cell index first. */
size_t ld_gi_region_workspace_bytes(const ld_geom_t* geom);
int ld_gi_region(const ld_geom_t* geom, const ld_loss_hp_t* hp, const ld_maps_t* cls,
                 const ld_maps_t* reg, const ld_maps_t* t_cls, const ld_maps_t* t_reg,
                 int topn, float iou_thr, float* im, int32_t* counts, void* workspace,
                 size_t workspace_bytes, ld_stream_t stream);

/* losses: device float[8 * num_levels], key-major (loss_cls[0..L), ...). */
int ld_loss_finalize(const ld_geom_t* geom, const ld_loss_hp_t* hp,
                     const int32_t* counts, const float* norm,
                     const void* workspace, float* losses, ld_stream_t stream);

/* The north-star kernel on its own, at any size: LD KL (T) + Integral
 * (+ fused gradient) over `rows`-many anchors x 4 sides, channel-major
 * (68, rows) student and teacher logits, weight (rows).
 *   integral (4, rows) out, loss_rows (4, rows) out = weight * KL per side,
 *   grad (68, rows) out or NULL (forward only).
 * Algorithmic bytes per anchor-side row: 136 logits in + 4 weight + 4 integral
 * + 4 loss (+ 68 gradient) = 148 forward / 216 fused forward+gradient.
 * Replaces Integral.forward (gfl_head.py:32-44) +
 * knowledge_distillation_kl_div_loss (kd_loss.py:10-36) on the dense map. */
int ld_kl_integral_dense(const float* s_reg, const float* t_reg,
                         const float* weight, int64_t rows, float T,
                         float scale, float* integral, float* loss_rows,
                         float* grad, ld_stream_t stream);

/* ---- reference-layout loss operators (row-major (rows, K) tensors) -------
 * These back the registry loss modules when they are called on their own,
 * with the reference's tensor layout.  Each computes the per-row loss
 * (already multiplied by weight[row] if weight != NULL) and, if grad != NULL,
 * d(sum_rows loss_rows * gscale)/d pred. */
/* knowledge_distillation_kl_div_loss, kd_loss.py:10-36 */
int ld_kd_kl_rows(const float* pred, const float* soft, const float* weight,
                  int64_t rows, int K, float T, float gscale, float* loss_rows,
                  float* grad, ld_stream_t stream);
/* quality_focal_loss, gfocal_loss.py:8-50 (beta = 2) */
int ld_qfl_rows(const float* pred, const int64_t* label, const float* score,
                const float* weight, int64_t rows, int C, float gscale,
                float* loss_rows, float* grad, ld_stream_t stream);
/* distribution_focal_loss, gfocal_loss.py:53-74 */
int ld_dfl_rows(const float* pred, const float* target, const float* weight,
                int64_t rows, int K, float gscale, float* loss_rows,
                float* grad, ld_stream_t stream);
/* giou_loss, iou_loss.py:85-102 (aligned boxes (rows, 4)) */
int ld_giou_rows(const float* pred, const float* target, const float* weight,
                 int64_t rows, float eps, float gscale, float* loss_rows,
                 float* grad, ld_stream_t stream);
/* iou_loss (iou_loss.py:14-36; linear != 0: 1 - IoU instead of -log IoU),
 * diou_loss (:107-157), ciou_loss (:162-219); eps = the module's */
int ld_iou_rows(const float* pred, const float* target, const float* weight,
                int64_t rows, float eps, int linear, float gscale,
                float* loss_rows, float* grad, ld_stream_t stream);
int ld_diou_rows(const float* pred, const float* target, const float* weight,
                 int64_t rows, float eps, float gscale, float* loss_rows,
                 float* grad, ld_stream_t stream);
int ld_ciou_rows(const float* pred, const float* target, const float* weight,
                 int64_t rows, float eps, float gscale, float* loss_rows,
                 float* grad, ld_stream_t stream);
/* l1_loss / smooth_l1_loss, smooth_l1_loss.py:9-56, ELEMENT-wise: pred, target,
 * weight (nullable), loss and grad all hold n floats; loss[i] = weight[i] *
 * l(pred[i] - target[i]), grad[i] = gscale * weight[i] * l'(...) (0 at a zero
 * difference; |d| < beta takes the quadratic branch, |d| == beta the linear). */
int ld_l1_rows(const float* pred, const float* target, const float* weight,
               int64_t n, float gscale, float* loss, float* grad,
               ld_stream_t stream);
int ld_smooth_l1_rows(const float* pred, const float* target, const float* weight,
                      int64_t n, float beta, float gscale, float* loss,
                      float* grad, ld_stream_t stream);
/* DeltaXYWHBBoxCoder.encode / decode (bbox2delta / delta2bbox,
 * delta_xywh_bbox_coder.py:87-237) on (rows, 4) boxes.  decode: max_hw =
 * host float[2] (height, width) clips the boxes to [0, w] x [0, h]; NULL = no
 * clip (max_shape=None or clip_border=False). */
int ld_delta_encode_rows(const ld_delta_t* delta, const float* boxes,
                         const float* gt, int64_t rows, float* deltas,
                         ld_stream_t stream);
int ld_delta_decode_rows(const ld_delta_t* delta, const float* boxes,
                         const float* deltas, int64_t rows, const float* max_hw,
                         float* out, ld_stream_t stream);
/* Integral.forward, gfl_head.py:32-44: (rows, 4*(reg_max+1)) -> (rows, 4);
 * backward: grad_in (rows,4) -> grad (rows, 68) */
int ld_integral_rows(const float* x, int64_t rows, float* out,
                     ld_stream_t stream);
int ld_integral_rows_bwd(const float* x, const float* grad_out, int64_t rows,
                         float* grad_x, ld_stream_t stream);
/* bbox_overlaps, iou2d_calculator.py:43-188; mode 0 iou, 1 iof, 2 giou,
 * 3 diou; pairwise (m, n) or aligned (m). */
int ld_bbox_overlaps(const float* b1, const float* b2, int64_t m, int64_t n,
                     int mode, int aligned, float eps, float* out,
                     ld_stream_t stream);
/* sum of a float vector into out[0] (deterministic two-stage) */
int ld_sum(const float* x, int64_t n, float* out, void* workspace,
           size_t workspace_bytes, ld_stream_t stream);

/* ---- convolution (fp32, implicit GEMM on the f32 matrix cores) -----------
 * Replaces nn.Conv2d under ResNet / FPN / GFLHead:
 *   backbones/resnet.py:35-46,163-183 (BasicBlock/Bottleneck convs),
 *   models/utils/res_layer.py:38-59 (downsample), necks/fpn.py:121-160,
 *   dense_heads/gfl_head.py:102-133.
 * Activations are (N, C, P) fp32 with P = sum over levels of H_l*W_l: a plain
 * NCHW tensor is the one-level case; the FPN/head use the level-concatenated
 * form so weight-shared convs over all five levels are one launch. */
typedef struct {
  int32_t Hin, Win, Hout, Wout;
  int32_t off_in, off_out; /* first position of the level inside Pin / Pout */
} ld_conv_level_t;

typedef struct {
  int32_t N, Cin, Cout, KH, KW;
  int32_t stride; /* 1 or 2 */
  int32_t pad;
  int32_t num_levels;
  int32_t Pin, Pout;
  ld_conv_level_t lv[LD_MAX_LEVELS];
} ld_conv_t;

/* Fused forward epilogue, applied in this order:
 *   v = acc; if scale: v = v*scale[co] + shift[co]  (frozen/eval BatchNorm,
 *   resnet.py:639-648); if bias: v += bias[co]; if residual: v += residual;
 *   if relu: v = max(v, 0).  Any pointer may be NULL.  (With y_raw: scale and
 *   bias together are not supported -- a conv followed by a norm has no bias.) */
typedef struct {
  const float* bias;
  const float* scale;
  const float* shift;
  const float* residual; /* same shape as y */
  int32_t relu;
  int32_t reserved;
  /* bf16 forward entry points only (NULL elsewhere): also write the final values
   * as the bf16 channel-blocked image (N, Cout/8, Pout, 8) of ld_conv_to_c8 --
   * bit-identical to converting y afterwards -- for the conv that consumes y
   * next.  Needs Cout % 8 == 0. */
  void* y_c8;
  /* bf16 forward entry points only: the residual as a C8 image instead of the
   * fp32 `residual` (give one or the other), and -- when y_c8 is given -- y
   * itself may be NULL: the frozen teacher then keeps ONLY the bf16 image of its
   * activations (the reference's mixed-precision nets are fp16 end to end the
   * same way, mmcv auto_fp16). */
  const void* residual_c8;
  /* Second output, same shape as y (forward entry points, MODE 0): the conv
   * result BEFORE scale / shift / residual / relu (acc + bias).  A trainable
   * conv -> eval-BN -> ReLU pair then runs as ONE launch: y is what the next
   * layer reads, y_raw is what the BN backward needs for d(gamma)
   * (resnet.py:639-648 keeps BN in eval mode; its affine stays trainable).
   * NULL = not written. */
  float* y_raw;
  /* ld_conv_bf16_forward_c8 only: that second output as a bf16 C8 image
   * (N, Cout/8, Pout, 8) instead of fp32 (give one or the other) -- what
   * ld_bn_act_backward_c8in reads for d(gamma); half the bytes (round 6). */
  void* y_raw_c8;
} ld_conv_epilogue_t;

/* (Cout,Cin,KH,KW) parameter -> GEMM images: wt_fwd [tap][Cin_pad][Cout]
 * and/or wt_bwd [KH*KW-1-tap][Cout_pad][Cin] (either may be NULL); *_pad = the
 * reduction extent rounded up to 32 rows, zero filled.  Image sizes in floats
 * come from ld_conv_weight_image_floats(..., backward = 0 | 1). */
size_t ld_conv_weight_image_floats(int Cout, int Cin, int KH, int KW,
                                   int backward);
int ld_conv_weight_transform(const float* w, int Cout, int Cin, int KH, int KW,
                             float* wt_fwd, float* wt_bwd, ld_stream_t stream);
/* Many weight images in ONE launch (after the optimizer step every trainable
 * conv of the student needs new images: 137 launches of a few microseconds
 * each otherwise).  `jobs` and `block_job` live in DEVICE memory; job j owns
 * the 256-thread blocks [first_block, first_block of job j+1); block_job[b] is
 * the job of block b.  wt_fwd / wt_bwd may be NULL per job. */
typedef struct {
  const float* w;
  float* wt_fwd;
  float* wt_bwd;
  int32_t Cout, Cin, ntaps, first_block;
} ld_wt_job_t;
int ld_conv_weight_transform_batch(const ld_wt_job_t* jobs, const int32_t* block_job,
                                   int nblocks, ld_stream_t stream);
/* The same images from 32 x 32 x ntaps channel tiles staged through LDS (round 5:
 * coalesced reads AND writes; the per-element kernels read the parameter with a
 * stride of Cin * ntaps floats -- 250 us per step for the R50 student).  A job owns
 * ld_conv_weight_transform_tiles(Cout, Cin, ntaps, bf16) consecutive blocks (0:
 * more than 9 taps, not served); bf16 != 0 writes the bf16 images of
 * ld_conv_bf16_weight_transform (wt_fwd / wt_bwd of the job then point at those).
 * Bit-identical to the per-element kernels. */
int ld_conv_weight_transform_tiles(int Cout, int Cin, int ntaps, int bf16);
int ld_conv_weight_transform_batch_tiled(const ld_wt_job_t* jobs,
                                         const int32_t* block_job, int nblocks, int bf16,
                                         ld_stream_t stream);
/* Enqueue only: no timing, no synchronisation, capturable into a hipGraph.
 * The tile shape of a launch comes from the tuning table (below) and, for a
 * geometry the table does not hold, from a model that is a pure function of the
 * geometry -- so two processes with the same table produce the same bits (the
 * KS = 4 split-K shapes sum in a different order than KS = 1). */
int ld_conv_forward(const ld_conv_t* c, const float* x, const float* wt_fwd,
                    const ld_conv_epilogue_t* ep, float* y, ld_stream_t stream);
/* dx (N,Cin,Pin) fully overwritten. */
int ld_conv_dgrad(const ld_conv_t* c, const float* dy, const float* wt_bwd,
                  float* dx, ld_stream_t stream);
/* dx = conv_transpose(dy) + addend, the sum formed in the GEMM epilogue.  addend
 * is (N,Cin,Pin) fp32 and may be dx itself.  Replaces the separate elementwise
 * add autograd issues wherever an activation has two consumers: the block input
 * of a residual block (mmdet/models/backbones/resnet.py:260-299: `out +=
 * identity`), a backbone stage output read by the next stage and the FPN lateral
 * (necks/fpn.py:170-176), an FPN level read by both head towers
 * (dense_heads/gfl_head.py:164-172).  Same tile shape (shape-table record) as
 * ld_conv_dgrad.  ld_conv_bf16_dgrad_acc / ld_conv_bf16_dgrad_c8_acc: the bf16
 * families. */
int ld_conv_dgrad_acc(const ld_conv_t* c, const float* dy, const float* wt_bwd,
                      const float* addend, float* dx, ld_stream_t stream);
/* ---- shape tuning (explicit; cudnn.benchmark's role, kept OUT of the launch
 * path).  ld_conv_tune_* time every candidate tile shape of the geometry by
 * launching the (idempotent) kernel on the caller's buffers -- y / dx must not
 * alias an input -- and record the winner: they synchronise the device and
 * must not be called on a capturing stream.  Return 0 = tuned now, 1 = the
 * geometry was already in the table (nothing done), < 0 / hipError_t on error.
 * ld_conv_tune_load merges a text table (one record per line: 18 key ints,
 * then tm tn wvm d ks; '#' comments) and returns the number of records;
 * ld_conv_tune_save writes the whole table; host paths. */
int ld_conv_tune_forward(const ld_conv_t* c, const float* x, const float* wt_fwd,
                         const ld_conv_epilogue_t* ep, float* y,
                         ld_stream_t stream);
int ld_conv_tune_dgrad(const ld_conv_t* c, const float* dy, const float* wt_bwd,
                       float* dx, ld_stream_t stream);
int ld_conv_tune_load(const char* path);
int ld_conv_tune_save(const char* path);
int ld_conv_tune_clear(void);
/* Lookups that found the record with this 18-int key since the last
 * ld_conv_tune_reset_hits (any launch or tune call that consulted the table);
 * -1 if the key is not in the table, LD_EINVAL for a null key.  Host paths. */
long long ld_conv_tune_hits(const int* key);
int ld_conv_tune_reset_hits(void);
/* Workspace of the plan a launch of this geometry actually follows (one size for
 * ld_conv_wgrad / ld_conv_bf16_wgrad / ld_conv_bf16_wgrad_c8).
 * ld_conv_tune_wgrad_workspace_bytes: the worst case over every candidate
 * ld_conv_tune_wgrad times (<= 128 MB), needed by that call only. */
size_t ld_conv_wgrad_workspace_bytes(const ld_conv_t* c);
size_t ld_conv_tune_wgrad_workspace_bytes(const ld_conv_t* c);
/* dw (Cout,Cin,KH,KW): overwritten, or += if accumulate != 0.  Deterministic:
 * the j-reduction is split in a fixed pattern (per wave, per k-group, per
 * workgroup) and every partial sum is combined in index order -- by a second
 * launch, or inside the launch by the last-arriving workgroup of a tile (no
 * float atomics either way).  Launches that may run concurrently must not share
 * a workspace. */
int ld_conv_wgrad(const ld_conv_t* c, const float* x, const float* dy, float* dw,
                  int accumulate, void* workspace, size_t workspace_bytes,
                  ld_stream_t stream);
/* Deferred reduction (round 5): a parameter gradient is needed when its bucket is
 * reduced across ranks / the optimizer runs, not when its layer's backward runs.
 * ld_conv_wgrad_partial computes only the split partials of a weight gradient --
 * family 0 = the fp32 kernels of ld_conv_wgrad, 1 = ld_conv_bf16_wgrad, 2 =
 * ld_conv_bf16_wgrad_c8 (x / dy as C8 images) -- into `slabs` (>=
 * ld_conv_wgrad_workspace_bytes(c), owned by this weight until the batch ran) and
 * fills job->slabs / splits / ntaps / Cout / Cin; the caller sets dw, accumulate
 * and first_block and uploads the jobs of a bucket once.  ld_wgrad_reduce_batch
 * sums every job of a table in ONE launch (block b serves 1024 consecutive
 * [tap][co][ci] elements of job block_job[b]; a job owns ceil(ntaps*Cout*Cin /
 * 1024) consecutive blocks from first_block): the same additions in the same
 * order as the per-layer reduce launch it replaces, 53 launches per step fewer. */
typedef struct {
  const float* slabs; /* [splits][ntaps][Cout][Cin] */
  float* dw;          /* (Cout, Cin, KH, KW) */
  int32_t splits, ntaps, Cout, Cin, accumulate, first_block;
} ld_wgrad_job_t;
int ld_conv_wgrad_partial(const ld_conv_t* c, int family, const void* x, const void* dy,
                          void* slabs, size_t slab_bytes, ld_wgrad_job_t* job,
                          ld_stream_t stream);
int ld_wgrad_reduce_batch(const ld_wgrad_job_t* jobs, const int32_t* block_job,
                          int nblocks, ld_stream_t stream);
/* The plan ld_conv_wgrad would follow for this geometry, without touching the
 * device: out[0..4] = kind (0 wave-private 64 x 64 tiles, 1 workgroup tiles, 2
 * three kw taps per workgroup), k-groups, columns per slice, splits along the
 * reduction, in-launch combination.  Order of precedence: LD_CONV_WGRAD_CFG, the
 * shape table (MODE 2), a model that is a pure function of the geometry. */
int ld_conv_wgrad_plan(const ld_conv_t* c, int* out);
/* ---- weight gradient of a small-Cin conv (the trainable stem) -----------------
 * The backward counterpart of ld_conv_forward_smallc: (ci, kh, kw) is ONE flat
 * GEMM dimension r < R = Cin*KH*KW (padded to 32 inside the kernel), dW[co][r] =
 * sum_j dY[co][j] * Xcol[r][j] on v_mfma_f32_32x32x2f32 with the input patch
 * staged through LDS (conv_wgrad_smallc.hip).  fp32 operands in either precision
 * mode.  Served geometries (ld_conv_wgrad_smallc_supported == 1): Cin < 16, R <=
 * 160, Cout 32 or 64, stride 1 or 2, one level; everything else LD_EUNSUPPORTED
 * (the caller keeps ld_conv_wgrad).  The reduction over j = (n, ho, wo) is cut
 * into ld_conv_wgrad_smallc_slabs(c) slabs (a function of the geometry alone);
 * each writes one partial laid out like dW into the workspace (>=
 * ld_conv_wgrad_smallc_workspace_bytes(c) = slabs * Cout * R * 4, else
 * LD_ENOSPACE before any launch), and the slabs are summed in slab order: no
 * atomics, two runs are bit-identical.
 *   ld_conv_wgrad_smallc          dw (Cout,Cin,KH,KW) overwritten, or += if
 *                                 accumulate != 0 (two launches: slabs, sum)
 *   ld_conv_wgrad_smallc_partial  the slabs only; fills job->slabs / splits /
 *                                 ntaps / Cout / Cin for ld_wgrad_reduce_batch as
 *                                 ld_conv_wgrad_partial does (the job describes the
 *                                 flat dW: ntaps = 1, Cout = 1, Cin = Cout * R);
 *                                 both forms give the same bits
 * There is no data gradient for these convs (the image needs none). */
int ld_conv_wgrad_smallc_supported(const ld_conv_t* c);
int ld_conv_wgrad_smallc_slabs(const ld_conv_t* c); /* < 0: LD_E* */
size_t ld_conv_wgrad_smallc_workspace_bytes(const ld_conv_t* c);
int ld_conv_wgrad_smallc(const ld_conv_t* c, const float* x, const float* dy, float* dw,
                         int accumulate, void* workspace, size_t workspace_bytes,
                         ld_stream_t stream);
int ld_conv_wgrad_smallc_partial(const ld_conv_t* c, const float* x, const float* dy,
                                 void* slabs, size_t slab_bytes, ld_wgrad_job_t* job,
                                 ld_stream_t stream);
/* Times the fp32 weight-gradient kernels / split shapes of this geometry on the
 * caller's buffers (dw is overwritten) and records the winner in the shape
 * table (key MODE 2).  Same rules and return values as ld_conv_tune_forward;
 * workspace_bytes >= ld_conv_tune_wgrad_workspace_bytes(c). */
int ld_conv_tune_wgrad(const ld_conv_t* c, const float* x, const float* dy, float* dw,
                       void* workspace, size_t workspace_bytes, ld_stream_t stream);

/* ---- convolution, bf16 matrix operands (BASELINE.json config 3) -----------
 * The same three GEMMs on v_mfma_f32_32x32x16_bf16 (16x the f32-MFMA rate).
 * Counterpart of the reference's mixed-precision mode for these layers (mmcv
 * auto_fp16 around ResNet / FPN / GFLHead forward; the reg output is cast back
 * by .float(), gfl_head.py:181-183; the loss block is @force_fp32,
 * ld_head.py:284).  Contract: x / dy / y / dx / dw, the epilogue operands and
 * the accumulators are fp32 exactly as in the fp32 entry points; only the two
 * MFMA operands are rounded to bf16 (round-to-nearest-even) on the way in.
 * Weight images: wt_fwd bf16 [tap][Cin16/8][Cout][8], wt_bwd bf16
 * [KH*KW-1-tap][Cout16/8][Cin][8] (C16 = channels rounded up to 16, zero
 * filled), sizes in bf16 ELEMENTS from ld_conv_bf16_weight_image_elems.
 * forward needs Cin % 16 == 0, dgrad Cout % 16 == 0 (LD_EUNSUPPORTED otherwise:
 * use the fp32 entry point); wgrad takes any channel counts and the workspace of
 * ld_conv_wgrad_workspace_bytes.  ld_conv_bf16_tune_* = ld_conv_tune_* for the
 * bf16 kernel family (same table, family field 1). */
size_t ld_conv_bf16_weight_image_elems(int Cout, int Cin, int KH, int KW,
                                       int backward);
int ld_conv_bf16_weight_transform(const float* w, int Cout, int Cin, int KH, int KW,
                                  void* wt_fwd, void* wt_bwd, ld_stream_t stream);
int ld_conv_bf16_weight_transform_batch(const ld_wt_job_t* jobs,
                                        const int32_t* block_job, int nblocks,
                                        ld_stream_t stream);
int ld_conv_bf16_forward(const ld_conv_t* c, const float* x, const void* wt_fwd,
                         const ld_conv_epilogue_t* ep, float* y, ld_stream_t stream);
int ld_conv_bf16_tune_forward(const ld_conv_t* c, const float* x, const void* wt_fwd,
                              const ld_conv_epilogue_t* ep, float* y,
                              ld_stream_t stream);
int ld_conv_bf16_dgrad(const ld_conv_t* c, const float* dy, const void* wt_bwd,
                       float* dx, ld_stream_t stream);
int ld_conv_bf16_tune_dgrad(const ld_conv_t* c, const float* dy, const void* wt_bwd,
                            float* dx, ld_stream_t stream);
int ld_conv_bf16_wgrad(const ld_conv_t* c, const float* x, const float* dy, float* dw,
                       int accumulate, void* workspace, size_t workspace_bytes,
                       ld_stream_t stream);
/* bf16 channel-blocked ("C8") activation operand.  ld_conv_to_c8 rewrites an
 * fp32 (N, C, P) tensor as bf16 (N, C/8, P, 8) (round to nearest even; C a
 * multiple of 8; `out` holds N*C*P bf16).  The *_c8 entry points take that
 * image as the activation operand of the forward conv (x_c8, Cin % 32 == 0) or
 * of the data gradient (dy_c8, Cout % 32 == 0) -- one 16-byte load per
 * (position, 8 channels), no conversion inside the GEMM loop; weights, the
 * fused epilogue and the fp32 (N, C, P) output are those of
 * ld_conv_bf16_forward / ld_conv_bf16_dgrad, and so are the results bit for
 * bit (the same bf16 operands enter the same fp32 accumulation order as the
 * LDS-tiled kernel of the fp32-input path).  LD_EUNSUPPORTED when the channel
 * count does not fit: use the fp32-input entry point. */
int ld_conv_to_c8(const float* x, int N, int C, int P, void* out, ld_stream_t stream);
int ld_conv_bf16_forward_c8(const ld_conv_t* c, const void* x_c8, const void* wt_fwd,
                            const ld_conv_epilogue_t* ep, float* y,
                            ld_stream_t stream);
int ld_conv_bf16_tune_forward_c8(const ld_conv_t* c, const void* x_c8,
                                 const void* wt_fwd, const ld_conv_epilogue_t* ep,
                                 float* y, ld_stream_t stream);
int ld_conv_bf16_dgrad_c8(const ld_conv_t* c, const void* dy_c8, const void* wt_bwd,
                          float* dx, ld_stream_t stream);
/* ---- launch lists ------------------------------------------------------------
 * Between ld_record_begin and ld_record_end every launch the calling thread makes
 * through this library is executed AND appended (kernel, grid, by-value copy of
 * its arguments) to a list; ld_record_replay re-issues the list on any stream with
 * one C loop -- no shape-table lookup, no descriptor building, no host language in
 * the per-launch path.  Everything a recorded launch points at (activations,
 * weight images, workspaces) must stay allocated while the list is used; tuning
 * entry points must not be called while recording.  ld_record_end returns a handle
 * > 0 (or a negative error); ld_record_count = launches in the list.  Used for the
 * frozen teacher's forward (mmdet/models/detectors/kd_one_stage.py:70-72: the same
 * ~150 launches on the same buffers every step). */
int ld_record_begin(void);
int64_t ld_record_end(void);
int ld_record_abort(void);
int ld_record_count(int64_t handle);
int ld_record_replay(int64_t handle, ld_stream_t stream);
int ld_record_free(int64_t handle);
/* ---- step lists: a captured hipGraph re-issued as plain stream launches ---------
 * ld_step_list_build walks the nodes of a captured hipGraph_t ONCE (kernel / memcpy
 * / memset parameters, dependency edges, capture order), assigns them to at most
 * max_lanes streams so that the capture's concurrency survives, and returns a
 * handle > 0 (negative: LD_EUNSUPPORTED for host / child-graph / allocation nodes,
 * LD_EINVAL otherwise).  ld_step_list_replay re-issues the step with one C loop of
 * hipLaunchKernel / hipMemcpyAsync / hipMemsetAsync calls (+ an event pair per
 * cross-lane edge): lane 0 is `stream`, the other lanes are streams the list owns;
 * they start behind everything enqueued on `stream` and `stream` ends up behind
 * them.  The graph and every buffer the captured step touched must outlive the
 * list.  ld_step_list_info: counts[8] = {kernel, memcpy, memset, ordering-only
 * nodes, lanes, cross-lane waits, nodes, cut marks}.  Nothing in the reference
 * (mmcv's runner issues every kernel from Python, mmdet/apis/train.py:74-127): what
 * takes the host language out of the student's ~350 launches per step. */
int64_t ld_step_list_build(void* hip_graph, int max_lanes);
/* Device-to-device copy as ONE kernel launch (16 bytes per lane): what a step that
 * will be captured uses instead of hipMemcpyAsync, whose captured 1-D memcpy node
 * this runtime cannot describe back to ld_step_list_build. */
int ld_copy_d2d(void* dst, const void* src, size_t bytes, ld_stream_t stream);
int ld_step_list_info(int64_t handle, int* counts);
int ld_step_list_replay(int64_t handle, ld_stream_t stream);
int ld_step_list_free(int64_t handle);
/* Cut marks: collectives BETWEEN the segments of a replay (a multi-process job; an
 * RCCL call inside a capture races with ProcessGroupNCCL's watchdog thread).  While
 * the step is captured, ld_step_list_mark(index, stream) stands where a collective
 * belongs: one launch of a marker kernel, index counting up from 0 per capture.
 * ld_step_list_build recognises the node by the kernel's address (LD_EINVAL if the
 * indices do not count up in list order) and counts it in counts[7];
 * ld_step_list_replay treats it as an ordering-only node.
 * ld_step_list_replay_until is the same replay in segments: with *cursor = 0 it
 * forks the lanes and issues the nodes in list order (capture order: the order the
 * eager step enqueued them in) up to the first mark, then returns *mark = its index,
 * *lane / *lane_stream = the lane it was captured on (lane 0 is `stream`).  That
 * stream is behind everything the mark depends on; what the caller enqueues on it
 * before the next call (the all-reduce, or the wait for one) is what the mark's
 * successors on every lane wait for.  Call again with the *cursor it left; the call
 * that runs off the end joins the lanes and returns *mark = -1, *cursor = 0.  Same
 * `stream` in every call of one replay; failures are reported as for
 * ld_step_list_replay (ld_step_list_last_failure). */
int ld_step_list_mark(int index, ld_stream_t stream);
int ld_step_list_replay_until(int64_t handle, ld_stream_t stream, int* cursor, int* mark,
                              int* lane, void** lane_stream);
/* debugging aid: the node the last failing replay stopped at: out8 = {node index,
 * hipGraphNodeType, hipError_t, lane, four type-specific details} */
int ld_step_list_last_failure(int* out8);
/* Stream `to` continues after everything enqueued on `from` so far (event record
 * + stream wait on a reusable per-device event): torch's
 * `side.wait_stream(main)` as one call.  Nothing in the reference: the fork of a
 * weight gradient onto the background stream of the backward pass.  Not on a
 * capturing stream. */
int ld_stream_fork(ld_stream_t from, ld_stream_t to);

/* ---- one frozen bottleneck as ONE launch (bf16 mode, C8-only activations) -----
 * y = relu(bn3(conv1x1(relu(bn2(conv3x3(relu(bn1(conv1x1(x)))))))) + x) for an
 * identity block (no downsample, stride 1) of a frozen ResNet trunk
 * (mmdet/models/backbones/resnet.py:260-299; the R101 teacher's layer3).  x_c8 /
 * y_c8: (N, Cin/8, H*W, 8) bf16 images (y_c8 != x_c8); w1 / w2 / w3: the bf16
 * forward images of the three convs (ld_conv_bf16_weight_transform: (mid, Cin, 1,
 * 1), (mid, mid, 3, 3), (Cin, mid, 1, 1)); scale / shift: the folded eval-BN
 * coefficients (ld_bn_prepare), 16-byte aligned.  The mid activations stay in
 * LDS; results are bit-identical to the three ld_conv_bf16_forward_c8 launches
 * with C8-only outputs.  ld_bottleneck_c8_supported: which widths the kernel is
 * built for (Cin 1024 / mid 256); LD_EUNSUPPORTED otherwise. */
typedef struct {
  int32_t N, H, W, Cin, mid, reserved;
  const void* w1;
  const void* w2;
  const void* w3;
  const float* scale1;
  const float* shift1;
  const float* scale2;
  const float* shift2;
  const float* scale3;
  const float* shift3;
} ld_bottleneck_t;
int ld_bottleneck_c8_supported(int Cin, int mid, int H, int W);
int ld_bottleneck_c8_forward(const ld_bottleneck_t* b, const void* x_c8, void* y_c8,
                             ld_stream_t stream);
int ld_conv_bf16_dgrad_acc(const ld_conv_t* c, const float* dy, const void* wt_bwd,
                           const float* addend, float* dx, ld_stream_t stream);
int ld_conv_bf16_dgrad_c8_acc(const ld_conv_t* c, const void* dy_c8, const void* wt_bwd,
                              const float* addend, float* dx, ld_stream_t stream);
int ld_conv_bf16_tune_dgrad_c8(const ld_conv_t* c, const void* dy_c8,
                               const void* wt_bwd, float* dx, ld_stream_t stream);
/* Weight gradient with BOTH operands as C8 images (Cin, Cout multiples of 8):
 * tile rows are positions (16-byte loads, aligned under any tap shift), the
 * position -> lane transpose the MFMA needs is done by ds_read_b64_tr_b16 in
 * the LDS read.  fp32 slabs / dw exactly as ld_conv_bf16_wgrad (same workspace
 * size); the per-element summation order differs from it. */
int ld_conv_bf16_wgrad_c8(const ld_conv_t* c, const void* x_c8, const void* dy_c8,
                          float* dw, int accumulate, void* workspace,
                          size_t workspace_bytes, ld_stream_t stream);

/* Small-Cin variant (the 7x7 stride-2 stem, resnet.py:558-570): flat
 * (ci,kh,kw) reduction; wt = [pad32(Cin*KH*KW)][Cout] image obtained with
 * ld_conv_weight_transform(w, Cout, Cin*KH*KW, 1, 1, wt, NULL). */
int ld_conv_forward_smallc(const ld_conv_t* c, const float* x, const float* wt,
                           const ld_conv_epilogue_t* ep, float* y,
                           ld_stream_t stream);

/* ---- normalisation / elementwise layers ----------------------------------
 * Level list of a level-concatenated (N, C, P) tensor (P = sum H_l*W_l). */
typedef struct {
  int32_t num_levels;
  int32_t H[LD_MAX_LEVELS];
  int32_t W[LD_MAX_LEVELS];
} ld_levels_t;

/* BatchNorm2d in eval mode (running stats frozen, affine trainable:
 * resnet.py:639-648, norm_cfg requires_grad=True): scale = gamma*rsqrt(var+eps),
 * shift = beta - mean*scale, rstd = rsqrt(var+eps) (rstd may be NULL). */
int ld_bn_prepare(const float* gamma, const float* beta, const float* mean,
                  const float* var, float eps, int C, float* scale, float* shift,
                  float* rstd, ld_stream_t stream);
/* The same for many BatchNorms in one launch (device-resident job table, as
 * ld_conv_weight_transform_batch). */
typedef struct {
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  float* scale;
  float* shift;
  float* rstd;
  float eps;
  int32_t C, first_block, reserved;
} ld_bn_job_t;
int ld_bn_prepare_batch(const ld_bn_job_t* jobs, const int32_t* block_job,
                        int nblocks, ld_stream_t stream);
/* y = act(x*scale[c] + shift[c] (+ residual)) on (N, C, P)
 * (Bottleneck/BasicBlock tails, resnet.py:65-92,260-299). */
int ld_bn_act_forward(const float* x, const float* residual, const float* scale,
                      const float* shift, int N, int C, int P, int relu, float* y,
                      ld_stream_t stream);
/* The same with the bf16 channel-blocked image of y as a side output (see
 * ld_gn_forward_c8); C % 8 == 0, P % 4 == 0, 16-byte aligned tensors. */
int ld_bn_act_forward_c8(const float* x, const float* residual, const float* scale,
                         const float* shift, int N, int C, int P, int relu,
                         float* y, void* y_c8, ld_stream_t stream);
size_t ld_bn_act_backward_workspace_bytes(int N, int C, int P);
/* dz = relu ? dy*(y>0) : dy; dx = dz*scale (may be NULL); dres = dz (may be
 * NULL); dgamma = sum dz*(x-mean)*rstd, dbeta = sum dz (either may be NULL). */
int ld_bn_act_backward(const float* dy, const float* y, const float* x,
                       const float* scale, const float* mean, const float* rstd,
                       int N, int C, int P, int relu, float* dx, float* dres,
                       float* dgamma, float* dbeta, int accumulate,
                       void* workspace, size_t workspace_bytes,
                       ld_stream_t stream);
/* The same with the bf16 channel-blocked image of dx as a side output (bf16
 * mode: dx feeds the conv's C8 data- / weight-gradient kernels directly, no
 * conversion launch).  C % 8 == 0, P % 4 == 0, 16-byte aligned tensors,
 * N * ceil(P / 256) <= 256 partial slots; LD_EUNSUPPORTED otherwise (use the
 * plain form + ld_conv_to_c8). */
int ld_bn_act_backward_c8(const float* dy, const float* y, const float* x,
                          const float* scale, const float* mean, const float* rstd,
                          int N, int C, int P, int relu, float* dx, void* dx_c8,
                          float* dres, float* dgamma, float* dbeta, int accumulate,
                          void* workspace, size_t workspace_bytes, ld_stream_t stream);
/* ld_bn_act_backward_c8 with the two saved activations given as bf16 C8 images
 * (N, C/8, P, 8) instead of fp32 tensors (round 6): y_c8 = the image of the
 * layer's output (only its sign is used, the ReLU mask; NULL without relu), x_c8 =
 * the conv result before the affine as written through
 * ld_conv_epilogue_t.y_raw_c8.  dx may be NULL (only dx_c8 is written).  8 instead
 * of 12 bytes read per element; d(gamma) sees the bf16-rounded conv result.  Needs
 * C % 8 == 0 and P % 2 == 0 (four positions per thread when P % 4 == 0, two
 * otherwise: the 25 x 42 stage). */
int ld_bn_act_backward_c8in(const float* dy, const void* y_c8, const void* x_c8,
                            const float* scale, const float* mean, const float* rstd,
                            int N, int C, int P, int relu, float* dx, void* dx_c8,
                            float* dres, float* dgamma, float* dbeta, int accumulate,
                            void* workspace, size_t workspace_bytes,
                            ld_stream_t stream);
/* Deferred finalisation (round 5, see ld_wgrad_reduce_batch): with accumulate ==
 * LD_GRAD_DEFER the two BN backward entry points above write only their
 * per-workgroup fp64 partials ([C][nsplit] pairs (sum dz, sum dz*xhat), nsplit =
 * ld_bn_act_backward_nsplit(N, C, P, c8), c8 = 0 for ld_bn_act_backward, 1 for
 * ld_bn_act_backward_c8, 2 for ld_bn_act_backward_c8in) into `workspace` -- which the caller
 * then owns until ld_bn_bwd_finalize_batch has summed every job of a bucket in ONE
 * launch (16 channels per block, a job owns ceil(C / 16) blocks from first_block;
 * the arithmetic of the per-layer finalize launch: 37 launches per step fewer).
 * dgamma / dbeta must be non-NULL in the deferring call (they request the
 * partials) and are not written by it. */
#define LD_GRAD_DEFER 2
typedef struct {
  const double* partial;
  float* dgamma;
  float* dbeta;
  int32_t C, nsplit, accumulate, first_block;
} ld_bn_fin_job_t;
int ld_bn_act_backward_nsplit(int N, int C, int P, int c8);
int ld_bn_bwd_finalize_batch(const ld_bn_fin_job_t* jobs, const int32_t* block_job,
                             int nblocks, ld_stream_t stream);
/* BatchNorm2d with BATCH statistics (norm_eval=False: resnet.py:639-648 leaves the
 * unfrozen stages' BN in training mode) on (N, C, P), M = N * P >= 2 values per
 * channel.  Forward: per-channel sum x, sum x^2 in fp64 (slice partials in the
 * workspace, one fixed-order final, no atomics); mean = s/M, rstd = 1/sqrt(q/M -
 * mean^2 + eps) (biased variance, formed in fp64), scale = gamma*rstd, shift = beta
 * - mean*scale, all four [C] fp32 outputs; then y = act(x*scale + shift (+
 * residual)) as ld_bn_act_forward.  With update_running != 0 the final launch also
 * sets running_mean = (1-m) running_mean + m mean, running_var = (1-m) running_var
 * + m var M/(M-1) (unbiased) and *num_batches_tracked += 1 (a device int64), m =
 * momentum; any of the three may be NULL.  16-byte loads iff P % 4 == 0 and the
 * tensors are 16-byte aligned.  LD_EINVAL (nothing launched) for M < 2 or a
 * workspace smaller than ld_bn_train_workspace_bytes(N, C, P). */
size_t ld_bn_train_workspace_bytes(int N, int C, int P);
int ld_bn_train_forward(const float* x, const float* residual, const float* gamma,
                        const float* beta, float eps, double momentum, int N, int C,
                        int P, int relu, int update_running, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked, float* y,
                        float* mean, float* rstd, float* scale, float* shift,
                        void* workspace, size_t workspace_bytes, ld_stream_t stream);
/* Backward of the above from its saved y, x and [C] scale / mean / rstd: dz = relu ?
 * dy*(y>0) : dy; dbeta = sum dz, dgamma = sum dz*xhat, xhat = (x-mean)*rstd (fp64
 * slice partials, fixed-order final; either may be NULL, the sums are formed
 * regardless); dx = scale*(dz - dbeta/M - xhat*dgamma/M) (NULL: skipped); dres = dz
 * (NULL: skipped).  accumulate: 0 overwrites dgamma / dbeta, 1 adds to them;
 * LD_GRAD_DEFER is refused (dx needs the finished sums in this call). */
int ld_bn_train_backward(const float* dy, const float* y, const float* x,
                         const float* scale, const float* mean, const float* rstd,
                         int N, int C, int P, int relu, float* dx, float* dres,
                         float* dgamma, float* dbeta, int accumulate, void* workspace,
                         size_t workspace_bytes, ld_stream_t stream);
/* db[c] = sum_{n,p} dy (conv bias gradient, fpn.py / gfl_cls / gfl_reg). */
int ld_bias_grad(const float* dy, int N, int C, int P, float* db, int accumulate,
                 ld_stream_t stream);
/* The same sum as [C][nsplit] fp64 partial pairs (sum, 0), nsplit =
 * ld_bias_grad_nsplit(N, C, P), for ld_bn_bwd_finalize_batch (a job with dgamma ==
 * NULL, dbeta = db): the bias gradients of a bucket are finalised with its norm
 * gradients in one launch. */
int ld_bias_grad_nsplit(int N, int C, int P);
int ld_bias_grad_partial(const float* dy, int N, int C, int P, void* partial,
                         size_t partial_bytes, ld_stream_t stream);
/* GroupNorm(G) (+ReLU) applied per FPN level of a level-concatenated tensor
 * (gfl_head.py:102-126: each level is normalised on its own).  mean/rstd:
 * (N, G, num_levels) outputs kept for the backward. */
size_t ld_gn_forward_workspace_bytes(const ld_levels_t* lv, int N, int G);
int ld_gn_forward(const ld_levels_t* lv, const float* x, const float* gamma,
                  const float* beta, int N, int C, int G, float eps, int relu,
                  float* y, float* mean, float* rstd, void* workspace,
                  size_t workspace_bytes, ld_stream_t stream);
size_t ld_gn_backward_workspace_bytes(const ld_levels_t* lv, int N, int C);
int ld_gn_backward(const ld_levels_t* lv, const float* dy, const float* y,
                   const float* x, const float* gamma, const float* mean,
                   const float* rstd, int N, int C, int G, int relu, float* dx,
                   float* dgamma, float* dbeta, int accumulate, void* workspace,
                   size_t workspace_bytes, ld_stream_t stream);
/* The same with a bf16 channel-blocked side output (see ld_conv_to_c8): y_c8 /
 * dx_c8 receive the (N, C/8, P, 8) bf16 image of the fp32 tensor written in the
 * same launch, for the bf16 conv that consumes it next.  The fp32 results are
 * bit-identical to ld_gn_forward / ld_gn_backward.  Needs C % 8 == 0, P % 4 == 0
 * and 16-byte aligned tensors (LD_EUNSUPPORTED otherwise). */
int ld_gn_forward_c8(const ld_levels_t* lv, const float* x, const float* gamma,
                     const float* beta, int N, int C, int G, float eps, int relu,
                     float* y, void* y_c8, float* mean, float* rstd, void* workspace,
                     size_t workspace_bytes, ld_stream_t stream);
int ld_gn_backward_c8(const ld_levels_t* lv, const float* dy, const float* y,
                      const float* x, const float* gamma, const float* mean,
                      const float* rstd, int N, int C, int G, int relu, float* dx,
                      void* dx_c8, float* dgamma, float* dbeta, int accumulate,
                      void* workspace, size_t workspace_bytes, ld_stream_t stream);
/* The lean form of ld_gn_backward_c8 (round 6, bf16 mode): y is not an operand --
 * the ReLU mask y > 0 is recomputed from x, mean, rstd, gamma, beta with the
 * forward's own expression (bit-identical to reading y back) -- and dx (fp32) may
 * be NULL when every consumer of the gradient takes the C8 image dx_c8.  18 instead
 * of 30 bytes of HBM traffic per element.  ld_gn_forward_c8 accepts y == NULL the
 * same way (only the C8 image of the output is written). */
int ld_gn_backward_c8_lean(const ld_levels_t* lv, const float* dy, const float* x,
                           const float* gamma, const float* beta, const float* mean,
                           const float* rstd, int N, int C, int G, int relu, float* dx,
                           void* dx_c8, float* dgamma, float* dbeta, int accumulate,
                           void* workspace, size_t workspace_bytes, ld_stream_t stream);
/* MaxPool2d(kernel 3, stride 2, pad 1) on rows = N*C planes (resnet.py:570). */
int ld_maxpool3x3s2(const float* x, int rows, int H, int W, float* y,
                    ld_stream_t stream);
/* Its gradient (the trainable stem, frozen_stages = -1): x (rows, H, W) the
 * forward input, dy (rows, Ho, Wo), dx (rows, H, W) with EVERY element written
 * (no memset).  A gather: each input pixel visits the at most 4 windows that
 * cover it and takes dy of those whose maximum it is; the maximum of a window
 * is its first in-bounds element in row-major (kh, kw) order that attains it
 * (torch's rule; ties are the normal case behind a ReLU), the padding is -inf,
 * the addends of a pixel are added in ascending (oh, ow) order in fp32: equal
 * to torch's CPU backward bit for bit.  No atomics; enqueue only, capturable.
 * 16-byte loads / stores iff W % 4 == 0 and x, dx are 16-byte aligned.  NaN
 * inputs are outside the contract, as for the forward. */
int ld_maxpool_3x3s2_backward(const float* x, const float* dy, int rows, int H, int W,
                             float* dx, ld_stream_t stream);
/* ---- Res2Net block glue (backbones/res2net.py:108-162) ----------------------
 * Everything between the convs of a Bottle2neck, one launch each, on `stream`,
 * nothing allocated or synchronised.  u is relu(bn1(conv1(x))) of shape
 * (N, C = scales*w, P); all tensors contiguous fp32.  Pools are a row-major fp32
 * sum followed by one IEEE division; pool backwards sum dy / divisor addends in
 * ascending (oh, ow) order; no atomics anywhere (runs are bit-identical).  The
 * 16-byte paths are taken only when every address they form is 16-byte aligned.
 * Null pointers / bad geometry: LD_EINVAL before any launch.
 *
 * ld_res2_gather: y (N, w, P) = u[:, slice*w : (slice+1)*w] (+ addend (N, w, P),
 *   or NULL): the operand of conv `slice` with the hierarchical add fused.  The
 *   block's backward uses it on d cat: d sp_i = d cat[:, slice i] (+ d x_{i+1}).
 * ld_res2_concat: y (N, 4w, Py) = cat(a, b, c, tail); a, b, c are (N, w, Py) and
 *   tail is slice `tslice` (width w) of t (N, Ct, Pt):
 *     LD_RES2_TAIL_COPY      Pt = Py = H*W, tail copied;
 *     LD_RES2_TAIL_POOL      t at H x W, y at Ho x Wo = floor((H-1)/stride)+1:
 *                            AvgPool2d(3, stride, padding=1), divisor 9;
 *     LD_RES2_TAIL_POOL_BWD  t at Ho x Wo, y at H x W: that pool's backward.
 *   The block's backward uses it to assemble d u from the three conv-input
 *   gradients and d cat (COPY, or POOL_BWD where the forward pooled).
 * ld_avgpool_ceil_*: AvgPool2d(k, k, ceil_mode=True, count_include_pad=False)
 *   of the avg_down shortcut on rows = N*C planes, H x W -> ceil(H/k) x
 *   ceil(W/k); a partial last window divides by its number of valid elements. */
#define LD_RES2_TAIL_COPY 0
#define LD_RES2_TAIL_POOL 1
#define LD_RES2_TAIL_POOL_BWD 2
int ld_res2_gather(const float* u, const float* addend, int N, int C, int w, int slice,
                   long long P, float* y, ld_stream_t stream);
int ld_res2_concat(const float* a, const float* b, const float* c, const float* t,
                   int N, int w, int Ct, int tslice, int H, int W, int stride, int mode,
                   float* y, ld_stream_t stream);
int ld_avgpool_ceil_forward(const float* x, long long rows, int H, int W, int k,
                            float* y, ld_stream_t stream);
int ld_avgpool_ceil_backward(const float* dy, long long rows, int H, int W, int k,
                             float* dx, ld_stream_t stream);
/* FPN top-down step (fpn.py:182-191): out = fine + nearest_up(coarse) with the
 * finer map's size as target; rows = N*C planes.  Backward: dfine = dout
 * (identity), dcoarse[q] = sum of dout over the fine cells that read q. */
int ld_upsample_add_forward(const float* fine, const float* coarse, int rows,
                            int Hf, int Wf, int Hc, int Wc, float* out,
                            ld_stream_t stream);
int ld_upsample_add_backward(const float* dout, int rows, int Hf, int Wf, int Hc,
                             int Wc, float* dcoarse, ld_stream_t stream);
/* ... + addend (the gradient the coarse map already holds from its other
 * consumer, the level's output conv; may be NULL; may be dcoarse itself). */
int ld_upsample_add_backward_acc(const float* dout, int rows, int Hf, int Wf, int Hc,
                                 int Wc, const float* addend, float* dcoarse,
                                 ld_stream_t stream);
/* Level packing for the shared head towers (gfl_head.py:164-172 applies the same
 * convs to every FPN level; here they run on ONE level-concatenated (N, C, P)
 * tensor): levels[l] = contiguous (rows, H_l*W_l) fp32, x3 = (rows, P), rows = N*C.
 * pack copies the levels into x3, unpack is its inverse (the backward): one
 * launch for all levels. */
int ld_pack_levels(const ld_levels_t* lv, const float* const* levels, int rows,
                   float* x3, ld_stream_t stream);
int ld_unpack_levels(const ld_levels_t* lv, const float* x3, int rows,
                     float* const* levels, ld_stream_t stream);
/* The same with the bf16 C8 image ((N, C/8, len, 8), see ld_conv_to_c8) of the
 * destination as a side output: x3_c8 for pack, levels_c8[l] for unpack; C % 8 == 0. */
int ld_pack_levels_c8(const ld_levels_t* lv, const float* const* levels, int N, int C,
                      float* x3, void* x3_c8, ld_stream_t stream);
int ld_unpack_levels_c8(const ld_levels_t* lv, const float* x3, int N, int C,
                        float* const* levels, void* const* levels_c8, ld_stream_t stream);
/* mmcv Scale per level (gfl_head.py:182): y = x * scales[level]. */
int ld_scale_levels_forward(const ld_levels_t* lv, const float* x,
                            const float* scales, int rows, float* y,
                            ld_stream_t stream);
size_t ld_scale_levels_backward_workspace_bytes(const ld_levels_t* lv);
int ld_scale_levels_backward(const ld_levels_t* lv, const float* dy, const float* x,
                             const float* scales, int rows, float* dx,
                             float* dscales, int accumulate, void* workspace,
                             size_t workspace_bytes, ld_stream_t stream);
/* Scale followed by the activation of FCOSHead's box branch
 * (fcos_head.py:145-153), all levels in one launch: with u = x * scales[level],
 *   LD_SCALE_ACT_EXP          y = exp(u)
 *   LD_SCALE_ACT_RELU         y = max(u, 0)            (norm_on_bbox, training)
 *   LD_SCALE_ACT_RELU_STRIDE  y = max(u, 0) * strides[level]   (eval mode)
 * ``strides``: host array of lv->num_levels ints, read only by RELU_STRIDE.
 * backward: dx = s * y' * dy and dscales[l] = sum over level l of x * y' * dy,
 * y' = y (EXP) or [u > 0] (* stride), the partial sums in fp64 and in the fixed
 * order of ld_scale_levels_backward (its workspace size; no float atomics).
 * ``y``: the forward output (read by EXP only, may be NULL otherwise). */
#define LD_SCALE_ACT_EXP 0
#define LD_SCALE_ACT_RELU 1
#define LD_SCALE_ACT_RELU_STRIDE 2
int ld_scale_act_levels_forward(const ld_levels_t* lv, const float* x,
                                const float* scales, const int32_t* strides, int mode,
                                int rows, float* y, ld_stream_t stream);
int ld_scale_act_levels_backward(const ld_levels_t* lv, const float* dy, const float* x,
                                 const float* y, const float* scales,
                                 const int32_t* strides, int mode, int rows, float* dx,
                                 float* dscales, int accumulate, void* workspace,
                                 size_t workspace_bytes, ld_stream_t stream);
/* torch.optim.SGD(momentum, weight_decay) over a flat parameter arena
 * (apis/train.py:88): d = g*grad_scale + wd*p; buf = mu*buf + d; p -= lr*buf. */
int ld_sgd_step(float* params, const float* grads, float* momentum_buf, size_t n,
                float lr, float momentum, float weight_decay, float grad_scale,
                ld_stream_t stream);
/* The same update with hyper = {lr, momentum, weight_decay, grad_scale} read
 * from DEVICE memory (bit-identical arithmetic): inside a captured hipGraph the
 * by-value arguments above are frozen, a buffer is not -- the host rewrites it
 * between replays (learning-rate schedules, apis/train.py:88 + lr hooks). */
int ld_sgd_step_dev(float* params, const float* grads, float* momentum_buf, size_t n,
                    const float* hyper, ld_stream_t stream);

/* ---- optimizer of a config's recipe (optim.hip, ld_amd/optim.py) ---------------
 * hyper (DEVICE, fp32) = {momentum, grad_scale, max_norm, 0,
 *                         lr_0, wd_0, lr_1, wd_1, ..., lr_{C-1}, wd_{C-1}}:
 * one (lr, weight_decay) pair per parameter class of mmcv's
 * DefaultOptimizerConstructor paramwise_cfg (bias_lr_mult, *_decay_mult,
 * custom_keys), C <= LD_SGD_MAX_CLASSES.  Read on the device, so a captured step
 * follows an lr schedule the host rewrites between replays. */
#define LD_SGD_MAX_CLASSES 64
/* torch.optim.SGD with per-class (lr, wd):
 *   d = g*s + wd_c*p; buf = mu*buf + d; p -= lr_c*buf,   s = grad_scale * clip[1]
 * (s = grad_scale when clip is NULL).  chunk_class: one uint8 class id per 64
 * floats of the arena (ceil(n / 64) entries; every parameter starts on a 64-float
 * boundary).  clip: NULL or the output of ld_grad_norm.  With one class and
 * clip[1] == 1 the result is bit-identical to ld_sgd_step / ld_sgd_step_dev. */
int ld_sgd_step_classes(float* params, const float* grads, float* momentum_buf,
                        size_t n, const uint8_t* chunk_class, int num_classes,
                        const float* hyper, const float* clip, ld_stream_t stream);
/* torch.nn.utils.clip_grad_norm_(max_norm, norm_type=2) of grads * grad_scale
 * (the arena holds the SUM over ranks; mmcv's OptimizerHook clips the average):
 * out = {total_norm, clip_coef}, total_norm = grad_scale * ||grads||_2,
 * clip_coef = min(1, max_norm / (total_norm + 1e-6)) in fp32.  fp64 partials of a
 * fixed grid, then one fixed-order final sum: the same bits on every run.  grad_scale
 * and max_norm come from hyper[1], hyper[2] (layout above). */
size_t ld_grad_norm_workspace_bytes(void);
int ld_grad_norm(const float* grads, size_t n, const float* hyper, float* out,
                 void* workspace, size_t workspace_bytes, ld_stream_t stream);

/* Virtual ranks (SGDTrainer(virtual_ranks=W)): out[c] = (table[0][c] + table[1][c] +
 * ... + table[W-1][c]) / W for c < n, rows row_stride floats apart (row_stride >= n).
 * fp32, summed in ascending rank order, then ONE division: the value all_reduce(SUM)
 * + div_(world) gives every rank of a W-process job.  One thread per column, no
 * atomics: the same bits on every run.  Serves the 2 loss normalisers
 * (ld_head.py:338-341, 362-365) and the logged values (base.py:211-214). */
int ld_vrank_reduce(const float* table, int W, int n, size_t row_stride, float* out,
                    ld_stream_t stream);

/* ---- GFLv2 distribution-guided quality branch (config 5, R-V2) ----------------
 * GFocalHead.forward_single's tail (gfocal_head.py:201-217) for all levels and
 * images in one launch, on the level-concatenated (N, C, P) tensors:
 *   prob = softmax over the 17 bins of each side of reg (N, 68, P)
 *   stat = [top-4 probabilities (descending), their mean] per side -> 20 values
 *   quality = sigmoid(w2 . relu(w1 stat + b1) + b2)       reg_conf, :140-144
 *   cls_score[c] = sigmoid(cls_feat[c]) * quality          (N, C, P)
 * w1 (64, 20) row-major, b1 (64), w2 (64), b2 (1); reg_topk = 4, add_mean,
 * reg_channels = 64 are compiled in.  quality (N, P) is kept for the backward.
 * Backward: g_cls_feat = g_cls_score * quality * sigma'(cls_feat);
 * g_reg (N, 68, P) through sigmoid, the MLP, top-k scatter and the softmax
 * (both fully overwritten); parameter gradients summed over all anchors in a
 * fixed order (per-block partials in the workspace), written or accumulated. */
int ld_quality_forward(const float* reg, const float* cls_feat, int N, int C, int P,
                       const float* w1, const float* b1, const float* w2,
                       const float* b2, float* cls_score, float* quality,
                       ld_stream_t stream);
size_t ld_quality_backward_workspace_bytes(int N, int P);
int ld_quality_backward(const float* reg, const float* cls_feat, const float* quality,
                        const float* g_cls_score, int N, int C, int P,
                        const float* w1, const float* b1, const float* w2,
                        const float* b2, float* g_cls_feat, float* g_reg,
                        float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                        int accumulate, void* workspace, size_t workspace_bytes,
                        ld_stream_t stream);

/* ---- measurement support: HBM streaming ceilings ------------------------------
 * Not on the train step.  bench.py times these in the same process as the
 * LD-KL kernel so its roofline fraction can be read against what the memory
 * system delivers for (a) a plain copy of n floats (width = 1 or 4 floats per
 * lane, nt = non-temporal access; 8 n bytes move) and (b) the LD-KL kernel's own
 * access pattern without its arithmetic: s, t, g are (68, rows) channel-major
 * maps, every (row, side) thread reads 17 + 17 planes and writes 17 (204 bytes
 * per row-side); side_fast = the four sides of a 256-row chunk in adjacent
 * workgroups (the mapping the train step's kernel uses). */
int ld_probe_copy(const float* src, float* dst, int64_t n, int width, int nt,
                  ld_stream_t stream);
int ld_probe_planes(const float* s, const float* t, float* g, int64_t rows, int nt,
                    int side_fast, ld_stream_t stream);

/* ---- grouped convolution, forward (config 5's X-101 teacher) ---------------------
 * The 3x3 conv2 of ResNeXt's Bottleneck (mmdet/models/backbones/resnext.py:49-61,
 * nn.Conv2d(width, width, 3, stride, padding=1, groups=32, bias=False)) and,
 * with K = 1, the grouped GEMM behind a grouped deformable conv (:62-74 over
 * ld_deform_im2col's columns).  x (N, Cin, Hin*Win), y (N, Cout, Hout*Wout)
 * fp32 NCHW; Cin % groups == Cout % groups == 0, Cout / groups in {4, 8, 16, 32},
 * K in {1, 3}.  wimage = ld_gconv_weight_transform of the PyTorch weight
 * (Cout, Cin/groups, K, K): [group][ci][tap][co], so the Cout/groups weights of
 * one (ci, tap) are consecutive dwords at a wave-uniform address (scalar loads).
 * Epilogue: y = relu?(scale[c] * acc + shift[c]) (eval-mode BN folded in; both
 * NULL = plain conv).  VALU kernel: 9-72 flop/B, HBM/L1-bound, not MFMA work. */
size_t ld_gconv_weight_image_floats(int Cout, int Cin, int groups, int K);
int ld_gconv_weight_transform(const float* w, int Cout, int Cin, int groups, int K,
                              float* image, ld_stream_t stream);
int ld_gconv_forward(const float* x, const float* wimage, float* y, int N, int Cin,
                     int Cout, int groups, int K, int stride, int pad, int Hin, int Win,
                     const float* scale, const float* shift, int relu,
                     ld_stream_t stream);

/* ---- grouped convolution, backward (the trainable ResNeXt teachers) -------------
 * fp32, single level, Cout / groups in {4, 8, 16, 32}, K in {1, 3}, stride in
 * {1, 2} (LD_EUNSUPPORTED otherwise); Cin / groups is free (9 * Cout / groups
 * for the K = 1 GEMM behind a grouped DCN).  No float atomics, no host
 * synchronisation, no allocation: two runs are bit-identical and every launch
 * can be captured.
 *
 * ld_gconv_dgrad: dx (N, Cin, Hin*Win) = the data gradient of ld_gconv_forward
 * for dy (N, Cout, Hout*Wout), as a gather (one thread per input position and
 * chunk of <= 32 of the group's input channels); addend non-NULL: dx = addend
 * + gradient (same shape as dx; may alias it).  wimage_bwd =
 * ld_gconv_weight_transform_bwd of the PyTorch weight:
 * [group][chunk][co][tap][c], ld_gconv_weight_image_bwd_floats floats (zero
 * padded to whole chunks).
 *
 * ld_gconv_wgrad: dw (Cout, Cin/groups, K, K) = (accumulate ? dw : 0) + the
 * weight gradient.  The N * Hout*Wout positions are cut into
 * ld_gconv_wgrad_slabs slabs (fixed size, per image); the first launch writes
 * one partial per (slab, element) into ``workspace`` (at least
 * ld_gconv_wgrad_workspace_floats floats, caller-owned), the second sums the
 * slabs in slab order. */
size_t ld_gconv_weight_image_bwd_floats(int Cout, int Cin, int groups, int K);
int ld_gconv_weight_transform_bwd(const float* w, int Cout, int Cin, int groups, int K,
                                  float* image, ld_stream_t stream);
int ld_gconv_dgrad(const float* dy, const float* wimage_bwd, const float* addend,
                   float* dx, int N, int Cin, int Cout, int groups, int K, int stride,
                   int pad, int Hin, int Win, ld_stream_t stream);
int ld_gconv_wgrad_slabs(int N, int K, int stride, int pad, int Hin, int Win);
size_t ld_gconv_wgrad_workspace_floats(int N, int Cin, int Cout, int groups, int K,
                                       int stride, int pad, int Hin, int Win);
int ld_gconv_wgrad(const float* x, const float* dy, float* dw, int accumulate,
                   float* workspace, size_t workspace_floats, int N, int Cin, int Cout,
                   int groups, int K, int stride, int pad, int Hin, int Win,
                   ld_stream_t stream);

/* ---- deformable convolution v1 (config 4's R101-DCN teacher; trainable) -------
 * mmcv.ops.DeformConv2dPack under resnet.py:171-194 (deform_groups = 1,
 * groups = 1).  ld_deform_im2col samples x (N, Cin, Hin, Win) bilinearly at
 * p*stride - pad + k*dilation + offset and writes the column tensor
 * col (N, Cin*KH*KW, Hout*Wout), channel = ci*KH*KW + k (= the order of
 * weight.view(Cout, Cin*KH*KW)); offset (N, 2*KH*KW, Hout, Wout) holds (dy, dx)
 * per tap, from the layer's own conv_offset 3x3 conv (ld_conv_forward).  The
 * product with the weights is ld_conv_forward as a 1x1 conv over Cin*KH*KW
 * channels.  Outside (-1, H) x (-1, W) the sample is 0; neighbours outside the
 * map contribute 0 (mmcv deform_conv_cuda_kernel.cuh; parity unpinned, the op
 * is not in the reference checkout). */
int ld_deform_im2col(const float* x, const float* offset, int N, int Cin, int Hin,
                     int Win, int KH, int KW, int stride, int pad, int dilation,
                     float* col, ld_stream_t stream);
/* Backward of the sampling (fp32; d_col (N, Cin*KH*KW, Hout*Wout) is the data
 * gradient of the 1x1 GEMM).  No float atomics: both results are bitwise
 * reproducible from run to run.
 * ld_deform_offset_grad: d_offset (N, 2*KH*KW, Hout*Wout), the analytic
 * derivative of the forward's four-term bilinear expression with the forward's
 * own floor (at an integer coordinate: the forward difference into the next
 * cell); 0 outside (-1, H) x (-1, W); a corner outside the map contributes 0.
 * Data gradient d_x (N, Cin, Hin*Win), in two calls that share one caller-owned
 * workspace of ld_deform_col2im_workspace_bytes (0: invalid geometry, or no
 * device to size the radix sort for):
 *   ld_deform_col2im_index  keys every (n, tap, position, corner) entry by the
 *     cell it touches, sorts the entries by cell (stable radix sort, hipcub, on
 *     `stream`) and finds each cell's segment; needs `offset` only and serves
 *     all Cin channels;
 *   ld_deform_col2im_sum    zeroes d_x, then sums every cell's segment in a
 *     fixed order (64-entry chunks of the sorted list, per-chunk partial sums
 *     added in chunk order for cells that cross chunk boundaries).
 * Nothing here allocates or synchronises; every launch goes to `stream`.
 * LD_EINVAL: bad arguments, or more than 2^31 entries / cells; LD_ENOSPACE:
 * workspace too small. */
int ld_deform_offset_grad(const float* x, const float* offset, const float* d_col, int N,
                          int Cin, int Hin, int Win, int KH, int KW, int stride, int pad,
                          int dilation, float* d_offset, ld_stream_t stream);
size_t ld_deform_col2im_workspace_bytes(int N, int Cin, int Hin, int Win, int KH, int KW,
                                        int stride, int pad, int dilation);
int ld_deform_col2im_index(const float* offset, int N, int Cin, int Hin, int Win, int KH,
                           int KW, int stride, int pad, int dilation, void* workspace,
                           size_t workspace_bytes, ld_stream_t stream);
int ld_deform_col2im_sum(const float* d_col, int N, int Cin, int Hin, int Win, int KH,
                         int KW, int stride, int pad, int dilation, void* workspace,
                         size_t workspace_bytes, float* d_x, ld_stream_t stream);

/* ---- modulated deformable convolution, DCNv2 (conv type 'DCNv2'; trainable) ---
 * mmcv.ops.ModulatedDeformConv2dPack, deform_groups = 1 (Zhu et al. 2019,
 * "Deformable ConvNets v2"; parity with mmcv UNPINNED: the op is in neither the
 * reference checkout nor on the build machine; checked against the float64
 * restatement tests/_mdcn_ref64.py).  `om` (N, 3*KH*KW, Hout, Wout) is the raw
 * output of the layer's conv_offset: channels [0, 2*KH*KW) are the offsets,
 * (dy, dx) interleaved per tap exactly as ld_deform_im2col's `offset`; channels
 * [2*KH*KW, 3*KH*KW) are the mask logits, one per tap.  No offset / mask tensor
 * is materialised: the kernels read the planes of `om` and take the sigmoid
 * themselves.
 *   col[n][ci*KH*KW + t][p] = sigmoid(logit_t(p)) * (v1's four-term bilinear sum)
 * with v1's window, floor, zero corners and term order; the mask multiplies the
 * finished sum, so with om = 0 col is exactly 0.5 x ld_deform_im2col's.
 * ld_mdeform_offset_mask_grad writes all 3*KH*KW channels of d_om in one launch
 * (one writer per element, every element written): the offset channels are v1's
 * expression times m, the logit channels m (1 - m) sum_ci d_col * (four-term
 * sum) -- exactly 0 where the sample is outside (-1, H) x (-1, W).
 * Data gradient: ld_mdeform_col2im_index is ld_deform_col2im_index with every
 * corner weight stored as weight * m.  The workspace layout is unchanged, so
 * ld_deform_col2im_workspace_bytes sizes it and ld_deform_col2im_sum consumes
 * it as they are (no float atomics; bitwise reproducible).
 * Return codes as the v1 entry points.  Measured once on an MI355X against the
 * v1 calls of the same shape (R101 c3-c5 conv2 at 2 x 800 x 1344; HIP events, v1
 * and v2 alternating in one process; tools/bench_mdcn.py ->
 * profiles/mdcn_latency.json): im2col 0.72-0.96 x, offset + mask gradient
 * 1.00-1.03 x, index 1.00-1.02 x, index + sum 1.00-1.01 x the v1 call. */
int ld_mdeform_im2col(const float* x, const float* om, int N, int Cin, int Hin, int Win,
                      int KH, int KW, int stride, int pad, int dilation, float* col,
                      ld_stream_t stream);
int ld_mdeform_offset_mask_grad(const float* x, const float* om, const float* d_col, int N,
                                int Cin, int Hin, int Win, int KH, int KW, int stride,
                                int pad, int dilation, float* d_om, ld_stream_t stream);
int ld_mdeform_col2im_index(const float* om, int N, int Cin, int Hin, int Win, int KH,
                            int KW, int stride, int pad, int dilation, void* workspace,
                            size_t workspace_bytes, ld_stream_t stream);

/* ---- device input pipeline ---------------------
 * Resize(keep_ratio) -> flip -> Normalize(to_rgb) -> Pad -> collate of the
 * reference's train_pipeline (configs/ld/ld_r18_gflv1_r101_fpn_coco_1x.py:66-77,
 * datasets/pipelines/transforms.py:203-233,416-450,524-580) for a whole batch in
 * one launch.  `imgs` is a DEVICE array of N descriptors; `data` points to a
 * decoded uint8 HWC image (3 channels, BGR as cv2.imread delivers) in device
 * memory; (new_h, new_w) is the resized size (mmcv.imrescale's rounding is host
 * logic: ld_amd/pipeline.py); `flip` = horizontal flip of the resized image.
 * out (N, 3, Hpad, Wpad) fp32, zeros beyond (new_h, new_w); mean / std_inv are
 * HOST float[3] in output-channel order (RGB when to_rgb).  Bilinear =
 * cv2 INTER_LINEAR on 8-bit data (11-bit fixed-point coefficients, rounded
 * uint8 result before normalisation). */
typedef struct {
  const unsigned char* data;
  int32_t src_h, src_w, new_h, new_w, flip, reserved;
} ld_image_t;
int ld_preprocess_batch(const ld_image_t* imgs, int N, int Hpad, int Wpad,
                        const float* mean, const float* std_inv, int to_rgb,
                        float* out, ld_stream_t stream);

/* ---- train-time augmentation in the same launch ----------------------------
 * Expand -> MinIoURandomCrop -> Resize -> RandomCrop -> RandomFlip -> Normalize
 * -> Pad (datasets/pipelines/transforms.py:916-1000, 1008-1140, 203-233,
 * 588-760, 416-450, 476-540) for a whole batch in one launch, with no
 * intermediate image.  Per image, all host decisions (ld_amd/pipeline.py):
 *   canvas  (canvas_h, canvas_w): Expand's canvas; the decoded image sits at
 *           (img_top, img_left), everything else is fill[c] (uint8, in the
 *           decoded image's BGR channel order).  No Expand: the image itself.
 *   window  (win_y, win_x, win_h, win_w) in canvas coordinates: what the resize
 *           reads (MinIoURandomCrop's patch; the whole canvas without it).
 *   resize  the window -> (new_h, new_w), the bilinear of ld_preprocess_batch
 *           with scale = win / new and source indices clamped to the WINDOW.
 *   crop    (crop_y, crop_x, out_h, out_w) in resized coordinates (RandomCrop);
 *           crop_y + out_h <= new_h, crop_x + out_w <= new_w.
 *   flip    horizontal, within the crop.
 * out (N, 3, Hpad, Wpad) fp32; outside (out_h, out_w) channel c holds
 * pad_val[c] as it is (Pad comes after Normalize).  mean / std_inv / pad_val are
 * HOST float[3] in output-channel order.  A descriptor with no canvas, the
 * full window, no crop and pad_val 0 gives ld_preprocess_batch's bits.
 * LD_EINVAL for a null pointer or a non-positive size; the descriptors are on
 * the device and are not inspected. */
typedef struct {
  const unsigned char* data;
  int32_t src_h, src_w;
  int32_t canvas_h, canvas_w, img_top, img_left;
  int32_t win_y, win_x, win_h, win_w;
  int32_t new_h, new_w;
  int32_t crop_y, crop_x, out_h, out_w;
  int32_t flip;
  unsigned char fill[4]; /* fill[0..2] = B, G, R; fill[3] unused */
} ld_image_aug_t;
int ld_preprocess_batch_aug(const ld_image_aug_t* imgs, int N, int Hpad, int Wpad,
                            const float* mean, const float* std_inv,
                            const float* pad_val, int to_rgb, float* out,
                            ld_stream_t stream);

/* ---- float-image mode: PhotoMetricDistortion in the same launch --------------
 * LoadImageFromFile(to_float32=True) -> PhotoMetricDistortion -> Expand ->
 * MinIoURandomCrop -> Resize -> RandomCrop -> RandomFlip -> Normalize -> Pad
 * (datasets/pipelines/transforms.py:810-902 and the steps above) for a whole
 * batch in one launch, with no intermediate image.  The geometry fields mean
 * what they mean in ld_image_aug_t; an output pixel walks back to four taps the
 * same way.  What differs:
 *   taps    a tap inside the image loads three bytes, converts them to fp32 and
 *           runs the photometric chain on that pixel; a tap on the canvas reads
 *           fill[] as it is (Expand comes after the distortion).
 *   chain   in the reference's order, every scalar a float32 rounded on the host:
 *             1  x += delta                       if do_brightness
 *             2  x *= alpha                       if do_contrast && contrast_mode == 1
 *             3  BGR -> HSV                       if do_hsv
 *             4  S *= saturation                  if do_saturation
 *             5  H += hue; H > 360: H -= 360; H < 0: H += 360    if do_hue
 *             6  HSV -> BGR                       if do_hsv
 *             7  x *= alpha                       if do_contrast && contrast_mode == 0
 *             8  x[c] = x[perm[c]]                (perm = 0, 1, 2: none)
 *           No clipping anywhere.  do_hsv = 0 (with do_saturation = do_hue = 0)
 *           is LoadImageFromFile(to_float32=True) without the distortion.
 *   HSV     restated from OpenCV's published float formulas, fp32 throughout:
 *             V = max(B, G, R); m = min(B, G, R); diff = V - m
 *             S = diff / (|V| + FLT_EPSILON); k = 60 / (diff + FLT_EPSILON)
 *             H = (G - B) * k             if V == R
 *                 (B - R) * k + 120       else if V == G
 *                 (R - G) * k + 240       else;          H < 0: H += 360
 *           and back: S == 0 gives B = G = R = V; else h = H * (6 / 360);
 *           h < 0: h += 6, else h >= 6: h -= 6; i = floor(h); f = h - i (i
 *           outside 0..5: i = 0, f = 0); tab = {V, V * (1 - S),
 *           V * (1 - S * f), V * (1 - S * (1 - f))}; (B, G, R) = tab[] at
 *           {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0} for i = 0 .. 5.
 *           The host keeps |hue| <= 360, so one wrap each way is enough.
 *   resize  cv2's float INTER_LINEAR: the same source index and fraction f as the
 *           8-bit path, coefficients 1 - f and f as floats, horizontal pass then
 *           vertical pass, no rounding to 8 bits.
 * Then BGR -> RGB when to_rgb and (v - mean) * std_inv; pad_val outside (out_h,
 * out_w).  Every operation is a correctly rounded fp32 + - * /, a compare, a
 * floor or an int conversion (built with -ffp-contract=off), so the output
 * equals the numpy float32 restatement in tests/_photometric_oracle.py bit for
 * bit.  Parity status: UNPINNED against cv2 itself (HSV conversions and float
 * resize); the order of the chain and the float32 scalar rounding are pinned on
 * the reference's own class (tests/golden/photometric.npz). */
typedef struct {
  const unsigned char* data;
  int32_t src_h, src_w;
  int32_t canvas_h, canvas_w, img_top, img_left;
  int32_t win_y, win_x, win_h, win_w;
  int32_t new_h, new_w;
  int32_t crop_y, crop_x, out_h, out_w;
  int32_t flip;
  float fill[3];      /* B, G, R of Expand's canvas, float32 */
  float delta, alpha, saturation, hue;
  int32_t do_brightness, do_contrast, contrast_mode, do_saturation, do_hue, do_hsv;
  int32_t perm[3];
  int32_t reserved;
} ld_image_photo_t;
int ld_preprocess_batch_photo(const ld_image_photo_t* imgs, int N, int Hpad, int Wpad,
                              const float* mean, const float* std_inv,
                              const float* pad_val, int to_rgb, float* out,
                              ld_stream_t stream);

/* ---- baseline JPEG decode, host half (LoadImageFromFile -> mmcv.imfrombytes ->
 * cv2.imdecode, datasets/pipelines/loading.py:12-71) -------------------------
 * The serial half of a JPEG decode: bytes -> int16 coefficient blocks, the input
 * of a device IDCT / upsampling / colour stage that is not in the library yet.
 *
 * No GPU call, no allocation; works in a process without a device:
 * marker parse and Huffman decode, from ITU-T T.81.  Supported: SOF0 / SOF1
 * (8-bit, Huffman), one interleaved scan; 1 component (any sampling) or 3
 * components YCbCr with luma 1x1, 2x1 or 2x2 and chroma 1x1; 8- and 16-bit DQT;
 * any DHT; DRI / RSTn; stuffing and fill bytes; APPn / COM skipped.
 * LD_EUNSUPPORTED, decided in the header before any entropy decoding
 * (info->message names the feature): progressive, lossless, hierarchical,
 * arithmetic coding, 12-bit, 4 components (CMYK / YCCK), Adobe transform 0
 * (RGB), other sampling factors, multi-scan baseline, DNL.  LD_EINVAL: anything
 * malformed or truncated (a Huffman code not in the table, more than 63 AC
 * positions in a block, a missing or out-of-sequence RSTn, premature end of
 * data, no EOI after the scan); libjpeg's pad-and-warn is not reproduced.
 *
 * Coefficient layout: per component, blocks in raster order over the
 * MCU-PADDED block grid (blocks_w x blocks_h; a single component is never
 * interleaved, its grid is ceil(w/8) x ceil(h/8)), 64 int16 each in natural
 * (row-major) order, NOT dequantised.  Component c starts at coef_off[c]. */
typedef struct {
  int32_t width, height, ncomp;
  int32_t hmax, vmax;              /* luma sampling factors (1 for 1 component) */
  int32_t restart_interval;        /* MCUs; 0 = none */
  int32_t mcus_x, mcus_y;
  int32_t h[4], v[4], tq[4];       /* per component: sampling, quant table id */
  int32_t blocks_w[4], blocks_h[4];/* MCU-padded block grid */
  int32_t plane_w[4], plane_h[4];  /* true component size, ceil(w*h_c/hmax) .. */
  int64_t coef_off[4];             /* in int16 elements */
  int64_t coef_count;              /* int16 elements of all components */
  int64_t coef_bytes;              /* 2 * coef_count */
  uint16_t quant[4][64];           /* PER COMPONENT, natural order */
  char message[64];                /* why a parse failed, NUL-terminated */
} ld_jpeg_info_t;
int ld_jpeg_parse(const unsigned char* bytes, size_t len, ld_jpeg_info_t* info);
/* `info` from ld_jpeg_parse of the same bytes; `coef` (host, pinned or not)
 * holds info->coef_count int16 and is written in full. */
int ld_jpeg_entropy_decode(const unsigned char* bytes, size_t len,
                           const ld_jpeg_info_t* info, int16_t* coef);
/* n images on min(n, 16, $LD_JPEG_THREADS, max_threads when >= 1) threads, never
 * sized by the machine.  status (may be NULL) receives each image's code. */
int ld_jpeg_entropy_decode_batch(const unsigned char* const* bytes, const size_t* lens,
                                 const ld_jpeg_info_t* infos, int16_t* const* coefs,
                                 int n, int max_threads, int* status);

/* ---- inference post-processing ---------------
 * GFLHead.get_bboxes for a whole batch (gfl_head.py:354-451 ->
 * post_processing/bbox_nms.py:70-195 -> mmcv.ops.batched_nms): sigmoid scores,
 * Integral * stride, per-level top-nms_pre by max class score, distance2bbox +
 * clamp to img_hw, optional division by scale_factors (rescale=True), score
 * threshold, class-aware greedy NMS (IoU > iou_thr suppresses), best
 * max_per_img (<= 1024) detections per image in descending score order.
 *   cls / reg      NCHW-direct head maps, (N, num_classes, H_l, W_l) /
 *                  (N, 4*(reg_max+1), H_l, W_l); reg_max must be 16
 *   img_hw         device (N, 2): img_shape height, width
 *   scale_factors  device (N, 4) or NULL
 *   dets           device (N, max_per_img, 5): x1, y1, x2, y2, score
 *   labels         device (N, max_per_img) int64;  counts device (N) int32
 * Equal scores: lower (anchor, class) index first.  iou_thr must be >= 0
 * (LD_EINVAL otherwise: a negative threshold suppresses across classes in the
 * reference's class-shift formulation).  Synchronises the stream once. */
size_t ld_get_bboxes_workspace_bytes(const ld_geom_t* g, int num_classes,
                                     int nms_pre);
int ld_get_bboxes(const ld_geom_t* g, const ld_maps_t* cls, const ld_maps_t* reg,
                  int num_classes, int reg_max, const float* img_hw,
                  const float* scale_factors, int nms_pre, float score_thr,
                  float iou_thr, int max_per_img, float* dets, int64_t* labels,
                  int32_t* counts, void* workspace, size_t workspace_bytes,
                  ld_stream_t stream);
/* The reference's optional nms type 'voting_cluster_diounms'
 * (post_processing/bbox_nms.py:141-176): same pipeline, but (1) the overlap
 * measure of the suppression is DIoU with the centre-distance term raised to
 * 0.8, evaluated on boxes shifted by 4000 * label as the reference shifts them
 * (Cluster-NMS iterated to its fixed point keeps exactly the boxes of the greedy
 * pass used here), and (2) score voting: every kept box is replaced by the
 * exp(-(1 - DIoU)^2 / 0.025) * score weighted mean of the candidates at or
 * below it in score order whose DIoU with it exceeds 0.7 (all other candidates
 * enter with the factor exp(-40), as in the reference's dense product).
 * Same arguments, workspace and outputs as ld_get_bboxes. */
int ld_get_bboxes_voting(const ld_geom_t* g, const ld_maps_t* cls, const ld_maps_t* reg,
                  int num_classes, int reg_max, const float* img_hw,
                  const float* scale_factors, int nms_pre, float score_thr,
                  float iou_thr, int max_per_img, float* dets, int64_t* labels,
                  int32_t* counts, void* workspace, size_t workspace_bytes,
                  ld_stream_t stream);
/* Both variants behind one entry point.  flags: LD_INFER_VOTING = the
 * score-voting Cluster-DIoU-NMS above; LD_INFER_PROB = the class maps already
 * hold probabilities and no sigmoid is applied -- GFocalHead.get_bboxes
 * (gfocal_head.py:317-596: cls_score = sigmoid(cls) * quality comes out of the
 * head, and num_classes = 81 there because use_sigmoid=False makes the
 * background column an ordinary score channel, anchor_head.py:68-71).
 * ``ctr`` (nullable): per-level (N, 1, H, W) centerness logits of ATSSGFLHead /
 * FCOSGFLHead (atss_gfl_head.py:420-575, fcos_gfl_head.py:347-546): the top-k
 * key becomes max_c score_c * sigmoid(centerness) and the factor multiplies
 * every candidate's score AFTER the score_thr test (multiclass_nms
 * score_factors, bbox_nms.py:114-123); not combinable with LD_INFER_VOTING.
 * LD_INFER_POINTS: decode about the FCOS points (x, y) * stride + stride / 2
 * (fcos_gfl_head.py:548-558) instead of the anchor centres (x, y) * stride.
 * ``num_base`` > 1 (RetinaGFLHead._get_bboxes, retina_gfl_head.py:301-412): the
 * maps are (N, num_base * C, H, W) / (N, num_base * 68, H, W); candidates are
 * the rows (cell, base anchor) in that order, top-k per level over all of
 * them, decoded about the shared cell centre.  Workspace: the _ex_ size.
 * LD_INFER_DELTA (ATSSHead / RetinaHead._get_bboxes, atss_head.py:376-508,
 * anchor_head.py:591-727): the reg maps are (N, num_base * 4, H, W) DeltaXYWH
 * deltas; a candidate is decoded with delta2bbox about its anchor and clipped to
 * img_shape (``delta``: the coder, required; ``anchors``: the explicit
 * (cells * num_base, 4) list in candidate-row order, or NULL with num_base = 1
 * for the square anchor of side anchor_scale * stride).  reg_max is ignored.
 * Everything around the decode -- keys, top-k, centerness factor, NMS, rescale
 * -- is unchanged.  Without the flag ``delta`` / ``anchors`` are not read.
 * LD_INFER_DIST (FCOSHead._get_bboxes, fcos_head.py:322-454; only with
 * LD_INFER_POINTS and num_base = 1, not with LD_INFER_DELTA): the reg maps are
 * (N, 4, H, W) distances in pixels; a candidate is distance2bbox(point, d,
 * max_shape=img_shape).  reg_max, ``delta`` and ``anchors`` are ignored;
 * everything around the decode is unchanged. */
#define LD_INFER_VOTING 1
#define LD_INFER_PROB 2
#define LD_INFER_POINTS 4
#define LD_INFER_DELTA 16 /* 8 is LD_AUG_RESCALE of ld_aug_merge_nms */
#define LD_INFER_DIST 32
size_t ld_get_bboxes_ex_workspace_bytes(const ld_geom_t* g, int num_classes,
                                       int num_base, int nms_pre);
int ld_get_bboxes_ex(const ld_geom_t* g, const ld_maps_t* cls, const ld_maps_t* reg,
                     const ld_maps_t* ctr, int num_classes, int num_base,
                     int reg_max, const float* img_hw,
                     const float* scale_factors, int nms_pre, float score_thr,
                     float iou_thr, int max_per_img, int flags,
                     const ld_delta_t* delta, const float* anchors, float* dets,
                     int64_t* labels, int32_t* counts, void* workspace,
                     size_t workspace_bytes, ld_stream_t stream);
/* get_bboxes(with_nms=False) of the same heads: stages 1-3 only (per-level top
 * nms_pre, Integral * stride, decode + clamp, optional rescale).  Outputs, per
 * image, the K = ld_get_bboxes_num_selected() rows in level order (within a
 * sorted level: descending key, as torch.topk returns them): boxes (N, K, 4),
 * scores (N, K, num_classes) WITHOUT the reference's zero background column,
 * and, with ``ctr``, the centerness factors (N, K).  Workspace: the _ex_ size. */
int ld_get_bboxes_num_selected(const ld_geom_t* g, int num_base, int nms_pre);
int ld_get_bboxes_pre_nms(const ld_geom_t* g, const ld_maps_t* cls,
                          const ld_maps_t* reg, const ld_maps_t* ctr,
                          int num_classes, int num_base, int reg_max,
                          const float* img_hw, const float* scale_factors,
                          int nms_pre, int flags, const ld_delta_t* delta,
                          const float* anchors, float* boxes, float* scores,
                          float* factors, void* workspace, size_t workspace_bytes,
                          ld_stream_t stream);

/* Test-time augmentation (BBoxTestMixin.aug_test_bboxes,
 * dense_test_mixins.py:38-100): one image seen through V views, each view's
 * get_bboxes(rescale=False, with_nms=False) rows (ld_get_bboxes_pre_nms) are
 * mapped back to the original image -- bbox_flip (transforms.py:5-30) in fp32,
 * then a true division by the view's scale_factor -- concatenated view-major
 * (merge_aug_bboxes) and passed through multiclass_nms with the concatenated
 * score factors (the factor multiplies a score AFTER its score_thr test).  The
 * merged set is not materialised; the candidate / NMS / voting stages are those
 * of ld_get_bboxes_ex.
 *   boxes         device (K, 4) in the view's image coordinates
 *   scores        device (K, score_stride) rows, the first num_classes used
 *                 (no background column)
 *   factors       device (K,) or NULL -- for every view or for none
 *   flip          LD_FLIP_*; img_h / img_w = the view's img_shape
 * flags: LD_INFER_VOTING (not with factors: LD_EUNSUPPORTED), LD_AUG_RESCALE =
 * rescale=True; without it the result is multiplied by view 0's scale_factor
 * (dense_test_mixins.py:94-98).  Outputs dets (max_per_img, 5), labels
 * (max_per_img) int64, count (1) int32, as ld_get_bboxes for one image.
 * max_per_img <= 1024 and iou_thr >= 0 as there.  Synchronises the stream once
 * (without LD_INFER_VOTING). */
#define LD_MAX_AUG_VIEWS 16
#define LD_FLIP_NONE 0
#define LD_FLIP_HORIZONTAL 1
#define LD_FLIP_VERTICAL 2
#define LD_FLIP_DIAGONAL 3
#define LD_AUG_RESCALE 8
typedef struct {
  const float* boxes;
  const float* scores;
  const float* factors;
  int32_t K, score_stride, flip, reserved;
  float img_h, img_w;
  float scale_factor[4];
} ld_aug_view_t;
size_t ld_aug_merge_nms_workspace_bytes(const ld_aug_view_t* views, int num_views,
                                        int num_classes);
int ld_aug_merge_nms(const ld_aug_view_t* views, int num_views, int num_classes,
                     float score_thr, float iou_thr, int max_per_img, int flags,
                     float* dets, int64_t* labels, int32_t* count, void* workspace,
                     size_t workspace_bytes, ld_stream_t stream);

/* ---- detection mAP evaluation (eval.hip) ----------------------------------
 * eval_map of the reference (core/evaluation/mean_ap.py) on the device.  One
 * batch of images: detections (n, 5) [x1 y1 x2 y2 score] with int64 labels, GTs
 * (g, 4) and ignored GTs (k, 4) with int64 labels, packed image after image;
 * *_off are DEVICE int32 arrays of num_imgs + 1 offsets.  All boxes fp32. */
#define LD_EVAL_MAX_SCALES 16
#define LD_EVAL_MAX_THRS 16
#define LD_EVAL_11POINTS 1 /* ld_eval_ap flags: average_precision '11points' */
typedef struct {
  const float* dets;
  const int64_t* det_labels;
  const int32_t* det_off;
  const float* gts;
  const int64_t* gt_labels;
  const int32_t* gt_off;
  const float* ign;
  const int64_t* ign_labels;
  const int32_t* ign_off;
  int32_t num_imgs, num_dets, num_gts, num_ign;
} ld_eval_batch_t;

/* tpfp_default for every (image, class), IoU threshold and area range of the
 * batch.  area_ranges: HOST fp32 [lo0, hi0, lo1, hi1, ...] (areas, i.e. the
 * squared scale bounds) or NULL for no range (num_scales must then be 1);
 * iou_thrs: HOST fp32, num_thrs <= LD_EVAL_MAX_THRS.  Writes num_dets * num_thrs
 * records, record d * num_thrs + t for detection d: the score, the segment
 * t * num_classes + label (num_thrs * num_classes for a label outside
 * [0, num_classes)), and bits: TP of scale k = bit k, FP = bit 16 + k.  Adds
 * the counted GTs of each (class, scale) to num_gts[class * num_scales + k]
 * (device int32, atomics: accumulate batches into one buffer). */
size_t ld_eval_tpfp_workspace_bytes(int num_dets);
int ld_eval_tpfp(const ld_eval_batch_t* batch, int num_classes, int num_scales,
                 const float* area_ranges, int num_thrs, const float* iou_thrs,
                 float* rec_score, int32_t* rec_seg, uint32_t* rec_bits, int32_t* num_gts,
                 void* workspace, size_t workspace_bytes, ld_stream_t stream);

/* Finalize every (threshold, class) segment of the records of all batches, in
 * the order they were written: stable sort by descending score, cumulative TP /
 * FP, recall (float64) and precision (fp32) into recall / precision
 * [num_scales][num_records] in sorted order, segment s = records
 * [seg_start[s], seg_start[s + 1]) (num_thrs * num_classes + 1 entries), and
 * ap[s * num_scales + k] ('area', or '11points' with LD_EVAL_11POINTS). */
size_t ld_eval_ap_workspace_bytes(int num_records, int num_scales);
int ld_eval_ap(int num_records, const float* rec_score, const int32_t* rec_seg,
               const uint32_t* rec_bits, int num_classes, int num_thrs, int num_scales,
               const int32_t* num_gts, int flags, int32_t* seg_start, double* recall,
               float* precision, float* ap, void* workspace, size_t workspace_bytes,
               ld_stream_t stream);

/* ---- per-image mAP ranking (eval_image.hip, eval.hip) ----------------------
 * bbox_map_eval of the reference (tools/analysis_tools/analyze_results.py:13-45)
 * for every image of a packed batch in ONE launch, one workgroup per image:
 * eval_map of that image alone (tpfp_default without area ranges, 'area' AP) at
 * each of iou_thrs (HOST float64, num_thrs <= LD_EVAL_MAX_THRS; the fp32 IoU is
 * compared with them in float64, so an fp32 comparison is its fp32 thresholds
 * widened), the float32 mean over the classes that have a non-ignored GT in
 * the image, then the float64 mean over the thresholds.  Writes
 *   ap[(i * num_thrs + t) * num_classes + c]  fp32, 0 for a class without GT
 *   has_gt[i * num_classes + c]               1 when image i has such a GT
 *   map[i]                                    float64, 0 for an image without GT
 * Sums follow numpy's pairwise order, so the results are the reference's bits.
 * Images whose boxes fit LDS (256 detections, 128 GTs + ignored GTs) stay there;
 * larger ones, or every image with LD_EVAL_IMAGE_NO_LDS, use the workspace. */
#define LD_EVAL_IMAGE_NO_LDS 1
size_t ld_eval_image_map_workspace_bytes(int num_dets, int num_imgs);
int ld_eval_image_map(const ld_eval_batch_t* batch, int num_classes, int num_thrs,
                      const double* iou_thrs, int flags, float* ap, uint8_t* has_gt,
                      double* map, void* workspace, size_t workspace_bytes,
                      ld_stream_t stream);

/* Stable ascending sort of num_imgs DEVICE float64 scores: order[k] is the
 * index of the k-th lowest score (equal scores keep index order), sorted[k] its
 * score.  Scores must not be NaN. */
size_t ld_rank_images_workspace_bytes(int num_imgs);
int ld_rank_images(int num_imgs, const double* scores, int32_t* order, double* sorted,
                   void* workspace, size_t workspace_bytes, ld_stream_t stream);

/* Paints rectangle outlines into img (DEVICE uint8, height x width x 3, in
 * place): the gt_boxes (g, 4) first, then the dets (m, 5) whose score >=
 * score_thr, each over what is already there.  Coordinates are truncated to
 * int32; a box covers x1..x2, y1..y2 inclusive and its outline is the band of
 * `thickness` pixels inside each edge; pixels outside the image are dropped.
 * Colors: channel 0 in bits 0-7, channel 1 in 8-15, channel 2 in 16-23. */
int ld_draw_boxes(uint8_t* img, int height, int width, const float* gt_boxes, int num_gts,
                  const float* dets, int num_dets, float score_thr, int thickness,
                  uint32_t gt_color, uint32_t det_color, ld_stream_t stream);

/* Paints text labels into img (DEVICE uint8, height x width x 3, in place) with
 * a fixed font for ASCII 0x20-0x7E: 5 x 7 glyphs at columns 1-5, rows 1-7 of a
 * 6 x 8 cell, the cell scaled by the integer `scale`.
 *   text_bytes  DEVICE, num_labels slots of LD_LABEL_MAX_LEN bytes; label i
 *               reads the first len_i bytes of slot i
 *   desc        DEVICE int32 (num_labels, 4): x1, y1, len, unused.  len is
 *               clamped to 0..LD_LABEL_MAX_LEN, x1 / y1 to +-2^30
 * Label i is a filled bg_color rectangle of len * 6 * scale by 8 * scale pixels
 * with the glyph pixels in fg_color; its top-left corner is (x1, y1 - 8 * scale)
 * when that row is >= 0, else (x1, y1).  A byte outside the font draws as '?',
 * len 0 draws nothing, pixels outside the image are dropped.  Where labels
 * overlap every pixel ends as if they were painted in index order: each pixel
 * takes the last label that covers it, so the result does not depend on
 * scheduling.  Colors as ld_draw_boxes.  LD_EINVAL on negative sizes or
 * scale < 1, LD_EUNSUPPORTED for scale > 1024; zero labels or pixels return 0
 * at once. */
#define LD_LABEL_MAX_LEN 64
int ld_draw_labels(uint8_t* img, int height, int width, const uint8_t* text_bytes,
                   const int32_t* desc, int num_labels, int scale, uint32_t fg_color,
                   uint32_t bg_color, ld_stream_t stream);

/* Row `row` (0-6, top first) of the glyph of character c (0x20-0x7E): five
 * bits, bit 4 the leftmost column; -1 outside those ranges.  Host only: it
 * reads the host copy of the table the kernel uses. */
int ld_font_glyph(int c, int row);

/* ---- proposal recall (recall.hip) -------------------------------------------
 * eval_recalls / _recalls of the reference (core/evaluation/recall.py:10-40,
 * 83-103).  One batch of images per ld_eval_recalls_match call: proposals
 * (k, prop_cols) fp32, prop_cols 5 = [x1 y1 x2 y2 score] or 4 = boxes already in
 * order, and GTs (g, 4) fp32, packed image after image; prop_off / gt_off are
 * DEVICE int32 arrays of num_imgs + 1 offsets.  max_img_props is a host bound:
 * the most proposals of one batch image.  proposal_nums: HOST int32, num_nums <=
 * LD_EVAL_RECALLS_MAX_NUMS, each >= 0; the proposals of an image are cut to
 * proposal_nums[num_nums - 1] (the LAST entry, as the reference does) after a
 * descending score sort (equal scores: the later index first).
 *
 * One workgroup per image computes the fp32 GT x proposal IoU tile and, for
 * every budget p, the reference's greedy matching over the first
 * min(k, proposal_nums[p]) columns.  Round j of image i writes
 *   gt_ious[p * gt_stride + gt_base + gt_off[i] + j]
 * the IoU of the GT matched in that round: -1 once the columns are used up, 0
 * for a budget without columns.  gt_ious is a DEVICE (num_nums, gt_stride) fp32
 * table that the caller grows batch after batch; gt_base is the number of GTs
 * of the batches before this one, gt_base + num_gts <= gt_stride.  Images
 * without GTs write nothing.  The tile stays in LDS when it fits (12288 IoUs,
 * 1024 kept proposals, 256 GTs); larger images, or every image with
 * LD_EVAL_RECALLS_NO_LDS, use the workspace.  Both routes give the same bits.
 * The host does not see the offsets, so the workspace (4-byte aligned,
 * ld_eval_recalls_workspace_bytes) is sized for the whole batch whichever route
 * its images take. */
#define LD_EVAL_RECALLS_MAX_NUMS 16
#define LD_EVAL_RECALLS_NO_LDS 1
size_t ld_eval_recalls_workspace_bytes(int num_props, int num_gts, int max_img_props,
                                       int cap);
int ld_eval_recalls_match(const float* props, int prop_cols, const int32_t* prop_off,
                          const float* gts, const int32_t* gt_off, int num_imgs,
                          int num_props, int num_gts, int max_img_props, int num_nums,
                          const int32_t* proposal_nums, int flags, float* gt_ious,
                          long long gt_stride, long long gt_base, void* workspace,
                          size_t workspace_bytes, ld_stream_t stream);

/* recalls[p * num_thrs + t] = count((double)gt_ious[p][g] >= iou_thrs[t], g <
 * total_gt) / (double)total_gt (DEVICE float64; iou_thrs HOST float64, num_thrs
 * <= LD_EVAL_MAX_THRS).  total_gt == 0 gives NaN, as the reference's division
 * does.  Integer counts, one writer per output: two runs give the same bits. */
int ld_eval_recalls_count(const float* gt_ious, long long gt_stride, long long total_gt,
                          int num_nums, int num_thrs, const double* iou_thrs,
                          double* recalls, ld_stream_t stream);

/* ---- COCO-style bbox evaluation (coco_eval.hip) ----------------------------
 * pycocotools' COCOeval(iouType='bbox') evaluate() + accumulate() as mmdet's
 * CocoDataset.evaluate runs them, float64 throughout.  Categories are indexed
 * in sorted category-id order (the K axis), images by their position in sorted
 * image-id order ("image rank").  One batch of images per ld_coco_match call:
 * detections (n, 5) fp32 [x1 y1 x2 y2 score] with int64 labels, packed image
 * after image (det_off: DEVICE int32, num_imgs + 1); img_rank: DEVICE int32 per
 * batch image; label_cat: DEVICE int32 label -> category index or -1 (not
 * scored).  The GTs of the whole dataset (num_all_imgs images), grouped by
 * (image rank, category index) in annotation order: cell c = rank * num_cats
 * + k holds GTs [gt_cell_off[c], gt_cell_off[c + 1]); xywh boxes and the json
 * area in float64, iscrowd 0/1, annotation ids.  max_img_dets / max_cell_gts
 * are host bounds: the most detections of one batch image, the most GTs of one
 * cell (<= LD_COCO_MAX_CELL_GTS). */
#define LD_COCO_MAX_THRS 16
#define LD_COCO_MAX_AREAS 4
#define LD_COCO_MAX_MAXDETS 4
#define LD_COCO_MAX_REC_THRS 128
#define LD_COCO_MAX_CELL_GTS 1024
typedef struct {
  const float* dets;
  const int64_t* labels;
  const int32_t* det_off;
  const int32_t* img_rank;
  const int32_t* label_cat;
  const double* gt_box;
  const double* gt_area;
  const int32_t* gt_crowd;
  const int64_t* gt_id;
  const int32_t* gt_cell_off;
  int32_t num_imgs, num_dets, num_labels, max_img_dets;
  int32_t num_all_imgs, num_cats, num_gts, max_cell_gts;
} ld_coco_batch_t;

/* evaluateImg for every (batch image, category) cell, every IoU threshold and
 * area range.  iou_thrs: HOST float64 (num_thrs), area_rng: HOST float64
 * [lo0, hi0, lo1, hi1, ...] (num_areas), num_thrs * num_areas <= 64; max_det:
 * maxDets[-1].  Writes one record per detection: score, category index
 * (num_cats when the label is not scored or its rank in its cell is
 * >= max_det), pos = image rank * max_det + rank in cell, and the 64-bit
 * matched (dtm != 0) / ignored (dtIg) masks, bit t * num_areas + a.  Adds the
 * non-ignored GTs of the batch images to npig[k * num_areas + a] (DEVICE int32,
 * atomics). */
size_t ld_coco_match_workspace_bytes(int num_dets, int max_img_dets, int max_det,
                                     int max_cell_gts);
int ld_coco_match(const ld_coco_batch_t* batch, int num_thrs, const double* iou_thrs,
                  int num_areas, const double* area_rng, int max_det, float* rec_score,
                  int32_t* rec_cat, uint32_t* rec_pos, uint64_t* rec_match,
                  uint64_t* rec_ign, int32_t* npig, void* workspace,
                  size_t workspace_bytes, ld_stream_t stream);

/* The matching of the reference's tools/analysis_tools/coco_error_analysis.py
 * (C75 / C50 / Loc rows plus the Sim and Oth passes of
 * analyze_individual_category).  The detection half is as ld_coco_batch_t's.
 * The GTs are grouped by image only: image rank r holds GTs
 * [gt_img_off[r], gt_img_off[r + 1]) in annotation order (DEVICE int32,
 * num_all_imgs + 1), at most max_img_gts (<= LD_COCO_MAX_CELL_GTS) per image;
 * gt_cat is each GT's category index, or -1 for a category outside the set;
 * cat_sup (DEVICE int32, num_cats) each category's supercategory index. */
typedef struct {
  const float* dets;
  const int64_t* labels;
  const int32_t* det_off;
  const int32_t* img_rank;
  const int32_t* label_cat;
  const double* gt_box;
  const double* gt_area;
  const int32_t* gt_crowd;
  const int64_t* gt_id;
  const int32_t* gt_cat;
  const int32_t* gt_img_off;
  const int32_t* cat_sup;
  int32_t num_imgs, num_dets, num_labels, max_img_dets;
  int32_t num_all_imgs, num_cats, num_gts, max_img_gts;
} ld_coco_err_batch_t;

/* ld_coco_match's records with num_thrs + 2 rows: row t < num_thrs is
 * evaluateImg at iou_thrs[t] (HOST float64); rows num_thrs ("Sim") and
 * num_thrs + 1 ("Oth") match at err_thr against the cell's own GTs plus the
 * image's GTs of the other categories of the same supercategory (Sim) or of
 * every other category (Oth), each taken as an ignored crowd GT of the cell's
 * category.  (num_thrs + 2) * num_areas <= 64.  npig counts the own GTs only,
 * as for ld_coco_match; ld_coco_accumulate with num_thrs + 2 thresholds then
 * gives every row. */
size_t ld_coco_match_errors_workspace_bytes(int num_dets, int max_img_dets, int max_det,
                                            int max_img_gts);
int ld_coco_match_errors(const ld_coco_err_batch_t* batch, int num_thrs,
                         const double* iou_thrs, double err_thr, int num_areas,
                         const double* area_rng, int max_det, float* rec_score,
                         int32_t* rec_cat, uint32_t* rec_pos, uint64_t* rec_match,
                         uint64_t* rec_ign, int32_t* npig, void* workspace,
                         size_t workspace_bytes, ld_stream_t stream);

/* accumulate() over the records of all batches: max_dets (HOST int32, sorted,
 * >= 1) and rec_thrs (HOST float64, ascending).  Writes precision and scores
 * [T][R][K][A][M] and recall [T][K][A][M] (DEVICE float64), -1 where npig is
 * 0. */
size_t ld_coco_accumulate_workspace_bytes(int num_records, int num_cats, int num_thrs,
                                          int num_areas, int num_max_dets);
int ld_coco_accumulate(int num_records, const float* rec_score, const int32_t* rec_cat,
                       const uint32_t* rec_pos, const uint64_t* rec_match,
                       const uint64_t* rec_ign, int num_cats, int num_all_imgs,
                       int num_thrs, int num_areas, int num_max_dets,
                       const int32_t* max_dets, int num_rec_thrs, const double* rec_thrs,
                       const int32_t* npig, double* precision, double* recall,
                       double* scores, void* workspace, size_t workspace_bytes,
                       ld_stream_t stream);

/* ---- AP landscape / teacher-student discrepancy (landscape.hip) ---------------
 * The reference's AP_landscape tool (detectors/single_stage.py:113-121,
 * apis/test.py:105-177) on the level-concatenated (N, C, P) fp32 tensors the
 * head towers consume (ld_pack_levels); `lv` lists the levels, whose H * W sum
 * to P.  Bad arguments (null pointers, K out of range, levels that do not fill
 * P, sizes <= 0) return LD_EINVAL before any launch.  No float atomics: two
 * calls on the same input give the same bits.
 *
 * ld_levels_mix: out[k * n + i] = coefs[2k] * own[i] + coefs[2k + 1] * other[i]
 * for the n elements of two tensors and 1 <= K <= LD_LEVELS_MIX_MAX_K grid
 * points (coefs: HOST, K pairs); out is (K, n), grid point major.  Two fp32
 * multiplies and one fp32 add in that order, never fused.  One launch; every
 * input element is read once. */
#define LD_LEVELS_MIX_MAX_K 16
int ld_levels_mix(const float* own, const float* other, long long n, int K,
                  const float* coefs, float* out, ld_stream_t stream);

/* out[n * num_levels + l] = sum over the positions p of level l of
 * (sum over c of |t[n, c, p] - s[n, c, p]|) / C (DEVICE float64): the
 * reference's abs(t - s).mean(1).sum() of one level and image.  The difference
 * and its absolute value are fp32, every sum is float64.  workspace: 8-byte
 * aligned, ld_levels_abs_err_workspace_bytes (0: bad arguments). */
size_t ld_levels_abs_err_workspace_bytes(const ld_levels_t* lv, int N, int C, int P);
int ld_levels_abs_err(const ld_levels_t* lv, const float* t, const float* s, int N, int C,
                      int P, double* out, void* workspace, size_t workspace_bytes,
                      ld_stream_t stream);

/* Pearson r of every row pair: a row is one (n, c) and the segment of one
 * level.  Two passes in float64 (means, then the centred sums), r = Sxy /
 * sqrt(Sxx * Syy).  A row with fewer than 2 positions, Sxx == 0 or Syy == 0 is
 * degenerate (torch gives NaN there) and left out.  r_sum[n * num_levels + l]
 * (DEVICE float64): the sum of r over the valid rows of (n, l);
 * counts[2 * (n * num_levels + l)] (DEVICE int32) their number, [.. + 1] the
 * number of degenerate rows.  workspace as for ld_levels_abs_err. */
size_t ld_levels_pearson_workspace_bytes(const ld_levels_t* lv, int N, int C, int P);
int ld_levels_pearson(const ld_levels_t* lv, const float* t, const float* s, int N, int C,
                      int P, double* r_sum, int32_t* counts, void* workspace,
                      size_t workspace_bytes, ld_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LD_HIP_H_ */
