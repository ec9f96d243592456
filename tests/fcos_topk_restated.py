"""Plain torch restatement of FCOSTopK's targets and losses (test infrastructure, no HIP), on top of oracle/.

    topk_targets       compute_targets_for_locations of slender_det/modeling/meta_arch/fcos/fcos_topk.py:24-101: the assignment of
                       oracle.fcos_targets plus, per gt box, its ``topk`` positive locations with the largest centerness target
    topk_losses        FCOSTopK.losses (fcos_topk.py:184-235) on flattened predictions
    OracleFCOSTopK     oracle.model.OracleFCOS whose training losses are the two above

The one place where the reference leaves the result open is a tie at the cut (``torch.topk(sorted=False)``, :86).  The rule here and
in the kernel: higher centerness first, then lower location index - a stable sort of the positives, which come in location order, by
descending centerness.
"""
import torch
import torch.nn.functional as F

from oracle import fcos_targets as ot
from oracle import losses as ol
from oracle.model import OracleFCOS


def select_topk(fg, gt_inds, ctr, num_gt, topk):
    """One image.  fg (L,) bool, gt_inds (L,) arg-min gt of every location, ctr (L,) centerness targets -> (L,) bool."""
    sel = torch.zeros_like(fg)
    for g in range(num_gt):
        rows = (fg & (gt_inds == g)).nonzero().squeeze(1)          # ascending location index
        if rows.numel() > topk:
            rows = rows[torch.sort(-ctr[rows], stable=True).indices[:topk]]
        sel[rows] = True
    return sel


def topk_targets(level_hw, strides, gt_boxes, gt_classes, radius, num_classes, topk=5):
    """-> labels (N, L) int64, reg (N, L, 4), ctr (N, L) (0 on background), gt_index (N, L) int64 into the concatenated gt list
    (-1 on background), sel (N, L) bool.  An image without gt is all background with nothing selected."""
    locs = ot.locations(level_hw, strides)
    pts = [len(l) for l in locs]
    allp = torch.cat(locs, dim=0)
    L = allp.shape[0]
    labs, regs, ctrs, inds, sels = [], [], [], [], []
    base = 0
    for b, c in zip(gt_boxes, gt_classes):
        b = b.float().reshape(-1, 4)
        if b.shape[0] == 0:
            lab, reg = ot.targets_for_image(allp, pts, strides, b, c, radius, num_classes)
            idx = torch.zeros(L, dtype=torch.int64)
        else:
            lab, reg, idx = ot.targets_for_image(allp, pts, strides, b, c, radius, num_classes, return_inds=True)
        fg = (lab >= 0) & (lab != num_classes)
        ctr = torch.zeros(L)
        ctr[fg] = ol.centerness_targets(reg[fg])
        labs.append(lab)
        regs.append(reg)
        ctrs.append(ctr)
        inds.append(torch.where(fg, idx + base, torch.full_like(idx, -1)))
        sels.append(select_topk(fg, idx, ctr, b.shape[0], topk))
        base += b.shape[0]
    return torch.stack(labs), torch.stack(regs), torch.stack(ctrs), torch.stack(inds), torch.stack(sels)


def topk_losses(labels, reg_targets, sel, cls_logits, box_pred, ctr_logits, num_classes, alpha, gamma, iou_type, world=1):
    """fcos_topk.py:184-235 on flattened rows: labels (M,), reg_targets (M, 4), sel (M,) bool, cls_logits (M, K), box_pred (M, 4) after
    exp / Scale, ctr_logits (M,).  Focal and centerness over all positives; IoU loss and its normaliser over ``sel``."""
    fg = (labels >= 0) & (labels != num_classes)
    pos_avg = max(int(fg.sum()) / float(world), 1.0)
    onehot = ol.one_hot_from_labels(labels, num_classes).to(cls_logits.dtype)
    cls_loss = ol.sigmoid_focal_loss(cls_logits, onehot, alpha, gamma, "sum") / pos_avg
    if int(fg.sum()) > 0:
        ctr_t = ol.centerness_targets(reg_targets[fg])
        ctr_sel = ol.centerness_targets(reg_targets[sel])
        reg_loss = ol.iou_loss_ltrb(box_pred[sel], reg_targets[sel], ctr_sel, iou_type) / (float(ctr_sel.sum()) / float(world))
        ctr_loss = F.binary_cross_entropy_with_logits(ctr_logits[fg], ctr_t, reduction="sum") / pos_avg
    else:
        reg_loss = box_pred[fg].sum()
        ctr_loss = ctr_logits[fg].sum()
    return {"cls_loss": cls_loss, "reg_loss": reg_loss, "centerness_loss": ctr_loss}


def permute_and_concat(pred_class_logits, pred_box_reg, pred_center_score, num_classes):
    """fcos/utils.py:32-52: per-level NCHW lists -> (N * L, K), (N * L, 4), (N * L,)."""
    def cat(ts, c):
        return torch.cat([t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, c) for t in ts], 1).reshape(-1, c)

    return cat(pred_class_logits, num_classes), cat(pred_box_reg, 4), cat(pred_center_score, 1).reshape(-1)


class OracleFCOSTopK(OracleFCOS):
    """OracleFCOS with FCOSTopK's targets and losses; ``last_labels`` / ``last_sel`` keep the (N, L) labels and selection of the
    last call."""
    topk_per_box = 5

    def losses(self, batched_inputs, world=1):
        c = self.c
        x = self.preprocess(batched_inputs)
        feats = self._fpn(self._bottom_up(x))
        level_hw = [tuple(f.shape[2:]) for f in feats]
        boxes = [b["instances"].gt_boxes.tensor.float().cpu() for b in batched_inputs]
        classes = [b["instances"].gt_classes.cpu() for b in batched_inputs]
        labels, reg_t, _ctr, _idx, sel = topk_targets(level_hw, c["strides"], boxes, classes, c["radius"], c["num_classes"], self.topk_per_box)
        self.last_labels, self.last_sel = labels, sel
        cls, box, ctr = self._head(feats)
        return topk_losses(labels.reshape(-1), reg_t.reshape(-1, 4).to(box.dtype), sel.reshape(-1), cls, box, ctr, c["num_classes"],
                           c["alpha"], c["gamma"], c["iou_type"], world)
