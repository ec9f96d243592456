"""RotatedRetinaNet: the one-stage dense detector on (cx, cy, w, h, angle_deg) boxes.

detectron2's rotated pieces in RetinaNet's slots - what the reference's in-tree copy slender_det/modeling/meta_arch/retina/retina_rotated.py
set out to be (Box2BoxTransformRotated at :71, RotatedBoxes.cat(anchors) at :271) before it stopped: it still matches with the axis-aligned
pairwise_iou (:276) and its head is 4 columns wide (:437).  There is no upstream model of this name; the semantics are:

  anchors   grid_anchors_rotated(level_hw, strides, SIZES, ASPECT_RATIOS, ANGLES, OFFSET), A = sizes x ratios x angles per location
  labels    Matcher(IOU_THRESHOLDS, IOU_LABELS, allow_low_quality_matches=True) over pairwise_iou_rotated(gt, anchors); matcher label
            0 -> K, -1 -> -1, 1 -> class of the matched gt; an image without gts: all K, all deltas 0
  targets   Box2BoxTransformRotated.get_deltas(anchor, matched gt), five weights, angle difference wrapped into [-180, 180)
  losses    RetinaNet's focal loss; smooth-L1 (SMOOTH_L1_LOSS_BETA) over the 5 deltas of the positives, or with BBOX_REG_LOSS_TYPE
            "rotated_iou" the sum of 1 - IoU(decoded box, matched gt) over the positives (the IoU the detector is scored by; no gradient
            for a positive whose decoded box does not overlap its gt), or with "rotated_giou" that sum plus (C - U) / C, C the area of
            the convex hull of the two boxes and U their union (such a positive then has the hull term's gradient, which pulls the box
            towards its gt), or with "rotated_kld" the sum of 1 - 1 / (1 + ln(1 + KL)) over the positives, KL the Kullback-Leibler
            divergence of the decoded box's Gaussian from its gt's (csrc/gauss_box_loss.h: smooth, a gradient without overlap, an angle
            gradient that grows with the squared aspect ratio; a square box's angle gets none); all / the EMA loss_normalizer
  inference per level sigmoid + threshold + top-k (dense_topk_select), Box2BoxTransformRotated.apply_deltas on the survivors, class-aware
            rotated NMS, top DETECTIONS_PER_IMAGE; Instances carry RotatedBoxes

MI355X-first: the whole batch is labelled by one kernel pair (sod_retina_label_rotated: 2 launches instead of 3 per image, no (R)
intermediates, the per-image gt counts stay on the device); the survivors are decoded by one launch (sod_retina_decode_rotated) instead
of a gather / index / where chain.  Backbone, towers, prediction convs, fused focal loss, normaliser, prefetch: RetinaNet's, shared through
RetinaNetBase; the class is deliberately no RetinaNet, so GeneralizedRCNNWithTTA (which un-flips XYXY boxes) refuses it as an unsupported class.
"""
import torch

from ...layers import functional as HF
from ..anchor_generator import grid_anchors_rotated
from ..postprocessing import batched_nms_instances
from .build import META_ARCH_REGISTRY
from .retinanet import RetinaNetBase


@META_ARCH_REGISTRY.register()
class RotatedRetinaNet(RetinaNetBase):
    box_dim = 5
    box_reg_loss_types = ("smooth_l1", "rotated_iou", "rotated_giou")
    gauss_box_reg_loss_types = ("rotated_kld",)

    def __init__(self, cfg):
        r, ag = cfg.MODEL.RETINANET, cfg.MODEL.ANCHOR_GENERATOR
        if ag.NAME != "RotatedAnchorGenerator":
            raise ValueError(f"RotatedRetinaNet: MODEL.ANCHOR_GENERATOR.NAME must be 'RotatedAnchorGenerator', got {ag.NAME!r}")
        if len(r.BBOX_REG_WEIGHTS) != 5:
            raise ValueError(f"RotatedRetinaNet: MODEL.RETINANET.BBOX_REG_WEIGHTS must hold five weights (dx, dy, dw, dh, da), got {tuple(r.BBOX_REG_WEIGHTS)}")
        if r.BBOX_REG_LOSS_TYPE not in self.box_reg_loss_types + self.gauss_box_reg_loss_types:
            raise ValueError(f"RotatedRetinaNet: MODEL.RETINANET.BBOX_REG_LOSS_TYPE must be 'smooth_l1', 'rotated_iou', 'rotated_giou' or 'rotated_kld', "
                             f"got {r.BBOX_REG_LOSS_TYPE!r}")
        A = self.num_cell_anchors(cfg)
        if A * r.NUM_CLASSES % 8:
            raise ValueError(f"RotatedRetinaNet: anchors per location ({A}, from MODEL.ANCHOR_GENERATOR.SIZES x ASPECT_RATIOS x ANGLES) times "
                             f"MODEL.RETINANET.NUM_CLASSES ({r.NUM_CLASSES}) must be a multiple of 8 (layout of the class-score buffer)")
        if any(int(l) not in (-1, 0, 1) for l in r.IOU_LABELS) or len(r.IOU_LABELS) != 3 or len(r.IOU_THRESHOLDS) != 2:
            raise ValueError("RotatedRetinaNet: MODEL.RETINANET.IOU_THRESHOLDS / IOU_LABELS must be two thresholds and three labels in {-1, 0, 1}")
        super().__init__(cfg)
        self.anchor_angles = [list(a) for a in ag.ANGLES]

    @staticmethod
    def num_cell_anchors(cfg):
        ag = cfg.MODEL.ANCHOR_GENERATOR
        return len(ag.SIZES[0]) * len(ag.ASPECT_RATIOS[0]) * len(ag.ANGLES[0])

    def anchors_for(self, level_hw):
        key = tuple(level_hw)
        if key not in self._anchor_cache:
            per_level = grid_anchors_rotated(level_hw, self.strides, self.anchor_sizes, self.anchor_ratios, self.anchor_angles, self.anchor_offset, self.device)
            self._anchor_cache[key] = torch.cat(per_level).contiguous()
        return self._anchor_cache[key]

    @torch.no_grad()
    def label_anchors(self, anchors, gt_instances):
        """-> gt_labels (N, R) int32 in {-1, 0..K-1, K} and gt_deltas (N, R, 5): two launches for the whole batch.  The gts are padded to
        the largest image's count from their shapes (known to the host); nothing is read back from the device.  For "rotated_iou", "rotated_giou" and "rotated_kld" the
        second output holds the matched gt boxes themselves (the loss compares decoded boxes with them); the labels do not change."""
        N = len(gt_instances)
        lens = [len(g) for g in gt_instances]
        Gmax = max(lens) if lens else 0
        dev = anchors.device
        boxes = torch.zeros((N, Gmax, 5), dtype=torch.float32, device=dev)
        classes = torch.zeros((N, Gmax), dtype=torch.int32, device=dev)
        if Gmax:
            slot = torch.tensor([i * Gmax + j for i, n in enumerate(lens) for j in range(n)], dtype=torch.int64).to(dev, non_blocking=True)
            boxes.view(-1, 5).index_copy_(0, slot, torch.cat([g.gt_boxes.tensor.float().view(-1, 5) for g in gt_instances]))
            classes.view(-1).index_copy_(0, slot, torch.cat([g.gt_classes.to(torch.int32).view(-1) for g in gt_instances]))
        counts = torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True)
        return HF.retina_label_rotated(anchors, boxes, classes, counts, self.iou_thresholds, self.iou_labels, True, self.num_classes,
                                       self.bbox_reg_weights, want_boxes=self.box_reg_loss_type in ("rotated_iou", "rotated_giou", "rotated_kld"))

    @torch.no_grad()
    def inference(self, level_hw, cls_buf, box_buf, offs, image_sizes):
        """Whole batch on the device: per level sigmoid over (HWA x K), top-k, score threshold (one selection launch), rotated decode of
        the survivors (one launch), class-aware rotated NMS and the top detections (batched NMS); the only host read is the final
        per-image detection count."""
        A, K = self.head.num_anchors, self.num_classes
        N, P = cls_buf.shape[:2]
        anchors = self.anchors_for(level_hw)
        rows_per_level = [h * w * A for h, w in level_hw]
        rows, scores, classes, _counts = HF.dense_topk_select(cls_buf.view(N, P * A, K), rows_per_level, K, self.score_threshold, self.topk_candidates)
        boxes = HF.retina_decode_rotated(box_buf, anchors, rows, scores, A, rows_per_level, self.topk_candidates, self.bbox_reg_weights, self.scale_clamp)
        return batched_nms_instances(boxes, scores, classes, self.nms_threshold, self.max_detections_per_image, image_sizes, box_dim=5)
