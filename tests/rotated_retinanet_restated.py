"""RotatedRetinaNet restated on the CPU from pieces the tests already trust: oracle.detection.pairwise_iou_rotated / matcher /
nms_rotated, oracle.rcnn.get_deltas / apply_deltas / anchors (their 5-column branches), oracle.losses.sigmoid_focal_loss /
smooth_l1_loss.  Semantics: detectron2's rotated pieces in RetinaNet's slots (modeling/meta_arch/rotated_retinanet.py).

``dtype``: the arithmetic after the IoU (thresholds, deltas, losses, decode) runs in it, so float64 serves as the arbiter.  The IoU itself is
oracle.detection's float32 emulation of detectron2's box_iou_rotated (a Python loop per pair: keep anchors x gts x images below ~1e4),
cast to ``dtype`` afterwards.
"""
import math

import torch

from oracle import detection as od
from oracle import losses as ol
from oracle import rcnn as orc

SCALE_CLAMP = math.log(1000.0 / 16)


def anchors(level_hw, strides, sizes, ratios, angles, offset=0.0, dtype=torch.float32):
    return torch.cat(orc.anchors(level_hw, strides, sizes, ratios, angles, offset)).to(dtype)


def iou_matrix(gt, anc, dtype=torch.float32):
    """(G, R) pairwise_iou_rotated(gt, anchors), clamped at 0 as the matcher sees it."""
    if len(gt) == 0:
        return torch.zeros((0, len(anc)), dtype=dtype)
    return od.pairwise_iou_rotated(gt.float(), anc.float()).clamp(min=0).to(dtype)


def label_anchors(anc, gt_boxes, gt_classes, thresholds, labels, num_classes, weights, dtype=torch.float32, ious=None):
    """anc (R, 5); per image gt_boxes (G, 5), gt_classes (G) -> gt_labels (N, R) int64 in {-1, 0..K-1, K}, gt_deltas (N, R, 5), and the
    per-image IoU matrices (for the margin analysis of the tests)."""
    out_l, out_d, out_q = [], [], []
    anc = anc.to(dtype)
    for i, (b, c) in enumerate(zip(gt_boxes, gt_classes)):
        q = iou_matrix(b, anc, dtype) if ious is None else ious[i]
        matches, mlab = od.matcher(q, thresholds, labels, True)
        if len(b):
            gl = c.long()[matches].clone()
            gl[mlab == 0] = num_classes
            gl[mlab == -1] = -1
            d = orc.get_deltas(anc, b.to(dtype)[matches], weights)
        else:
            gl = torch.full((len(anc),), num_classes, dtype=torch.int64)
            d = torch.zeros((len(anc), 5), dtype=dtype)
        out_l.append(gl)
        out_d.append(d)
        out_q.append(q)
    return torch.stack(out_l), torch.stack(out_d), out_q


def losses(pred_logits, pred_deltas, gt_labels, gt_deltas, num_classes, alpha, gamma, beta, normalizer, momentum=0.9):
    """pred_logits (N, R, K), pred_deltas (N, R, 5) -> ({loss_cls, loss_box_reg}, new EMA normaliser)."""
    valid = gt_labels >= 0
    pos = valid & (gt_labels != num_classes)
    normalizer = momentum * normalizer + (1 - momentum) * max(int(pos.sum()), 1)
    target = torch.nn.functional.one_hot(gt_labels[valid].long(), num_classes + 1)[:, :-1].to(pred_logits.dtype)
    loss_cls = ol.sigmoid_focal_loss(pred_logits[valid], target, alpha, gamma, "sum")
    loss_box = ol.smooth_l1_loss(pred_deltas[pos], gt_deltas.to(pred_deltas.dtype)[pos], beta, "sum")
    return {"loss_cls": loss_cls / normalizer, "loss_box_reg": loss_box / normalizer}, normalizer


def apply_deltas(deltas, boxes, weights):
    """Box2BoxTransformRotated.apply_deltas: oracle.rcnn's 5-column branch (dw, dh clamped at log(1000/16), angle wrapped into [-180, 180))."""
    return orc.apply_deltas(deltas, boxes, weights).view(-1, 5)


def inference_single_image(level_anchors, level_logits, level_deltas, num_classes, score_thresh, topk, nms_thresh, max_det, weights,
                           dtype=torch.float32):
    """Per level: sigmoid over (HWA x K), top-k, score threshold, rotated decode; then class-aware rotated NMS, top max_det.
    -> (kept candidate indices in order, candidate boxes (M, 5), scores (M), classes (M))."""
    B, S, C = [], [], []
    for anc, logit, delta in zip(level_anchors, level_logits, level_deltas):
        p = logit.reshape(-1).float().sigmoid()
        k = min(topk, delta.reshape(-1, 5).shape[0])         # retina_rotated.py:345: capped by the level's ANCHORS, not its anchor x class scores
        prob, idx = p.sort(descending=True, stable=True)
        prob, idx = prob[:k], idx[:k]
        keep = prob > score_thresh
        prob, idx = prob[keep], idx[keep]
        a = torch.div(idx, num_classes, rounding_mode="floor")
        if len(idx) == 0:         # no candidate of this level passes the threshold
            continue
        B.append(apply_deltas(delta.reshape(-1, 5).to(dtype)[a], anc.to(dtype)[a], weights))
        S.append(prob)
        C.append(idx % num_classes)
    if not B:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, 5, dtype=dtype), torch.zeros(0), torch.zeros(0, dtype=torch.int64)
    B, S, C = torch.cat(B), torch.cat(S), torch.cat(C)
    # class-aware: boxes of different classes never suppress each other - NMS per class on the unshifted boxes, merged in score order
    kept = torch.zeros(len(B), dtype=torch.bool)
    for c in C.unique().tolist():
        idx = torch.nonzero(C == c)[:, 0]
        kept[idx[od.nms_rotated(B[idx].float(), S[idx], nms_thresh)]] = True
    order = torch.sort(S, descending=True, stable=True).indices
    keep = order[kept[order]][:max_det]
    return keep, B, S, C
