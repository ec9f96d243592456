"""Plain torch restatement of FCOSRepPoints (slender_det/modeling/meta_arch/fcos/fcos_rpd_s1_topk.py) - test infrastructure, no HIP -
on top of oracle/ and tests/fcos_topk_restated.py.

    slender_centerness   compute_centerness_targets (:25-54): centerness WITHOUT the square root to the power min(w/h, h/w)
    slender_targets      compute_targets_for_locations (:57-134): the assignment of oracle.fcos_targets plus, per gt box, its ``topk``
                         positive locations with the largest slender centerness
    offsets2ltrb         FCOSRepPointsHead.offsets2ltrb (:709-745) and ``ltrb_rows`` / ``decode_boxes`` (:222-234)
    refine_targets       the second half of get_ground_truth (:343-374): pairwise_iou + Matcher per image on predicted boxes
    rpd_losses           FCOSRepPoints.losses (:249-317) on flattened rows
    decode_ltrb          inference_single_image's per-level part (:428-462) with the tie rule of sod_fcos_decode
    OracleFCOSRepPoints  oracle.model.OracleFCOS with the head of :505-707 and the pieces above

Where the reference leaves a result open, the rule here and in the kernels: a tie at the top-k cut goes to the higher score, then the
lower location index (as FCOSTopK); of two points that share an extremum ``torch.min`` / ``torch.max`` over the point dimension return
the FIRST (lowest index) on the CPU, which is the point the gradient goes to."""
import math

import torch
import torch.nn.functional as F

import fcos_topk_restated as TK
from oracle import detection as od
from oracle import fcos_targets as ot
from oracle import losses as ol
from oracle.deform_conv import deform_conv2d
from oracle.model import OracleFCOS, _relu_at

POINT_STRIDES = (1, 2, 4, 8, 16)          # offsets2ltrb's default argument (:709)


def slender_centerness(reg):
    lr, tb = reg[:, [0, 2]], reg[:, [1, 3]]
    q = (reg[:, 0] + reg[:, 2]) / (reg[:, 1] + reg[:, 3])
    r = torch.stack((q, 1 / q), dim=1).min(dim=1)[0]
    c = (lr.min(dim=-1)[0] / lr.max(dim=-1)[0]) * (tb.min(dim=-1)[0] / tb.max(dim=-1)[0])
    return torch.pow(c, r)


def slender_targets(level_hw, strides, gt_boxes, gt_classes, radius, num_classes, topk=5, score=slender_centerness):
    """-> labels (N, L) int64, reg (N, L, 4), score (N, L) (0 on background), gt_index (N, L) int64 into the concatenated gt list
    (-1 on background), sel (N, L) bool.  An image without gt is all background with nothing selected.  ``score``: the ranking score
    (``ol.centerness_targets`` gives FCOSTopK's selection on the same assignment)."""
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
        ctr[fg] = score(reg[fg])
        labs.append(lab); regs.append(reg); ctrs.append(ctr)
        inds.append(torch.where(fg, idx + base, torch.full_like(idx, -1)))
        sels.append(TK.select_topk(fg, idx, ctr, b.shape[0], topk))
        base += b.shape[0]
    return torch.stack(labs), torch.stack(regs), torch.stack(ctrs), torch.stack(inds), torch.stack(sels)


def offsets2ltrb(deltas, point_strides=POINT_STRIDES):
    """:709-745: per level (N, 2P, H, W) with channel 2k = x, 2k + 1 = y -> (N, 4, H, W) = (-min x, -min y, max x, max y)."""
    out = []
    for d, ps in zip(deltas, point_strides):
        N, C, H, W = d.shape
        pts = d.view(-1, C // 2, 2, H, W) * ps
        x, y = pts[:, :, 0], pts[:, :, 1]
        out.append(torch.cat([x.min(dim=1, keepdim=True)[0] * (-1), y.min(dim=1, keepdim=True)[0] * (-1),
                              x.max(dim=1, keepdim=True)[0], y.max(dim=1, keepdim=True)[0]], dim=1))
    return out


def ltrb_rows(per_level):
    """permute_to_N_HW_K + cat over the levels: list of (N, C, H, W) -> (N, L, C)."""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]) for t in per_level], 1)


def decode_boxes(ltrb, level_hw, strides):
    """:222-234: (N, L, 4) distances -> XYXY boxes around the FCOS locations."""
    loc = torch.cat(ot.locations(level_hw, strides)).to(ltrb.dtype)
    return torch.stack([loc[None, :, 0] - ltrb[..., 0], loc[None, :, 1] - ltrb[..., 1], loc[None, :, 0] + ltrb[..., 2], loc[None, :, 1] + ltrb[..., 3]], dim=2)


def refine_targets(level_hw, strides, init_boxes, gt_boxes, gt_classes, image_sizes, num_classes, thresholds=(0.4, 0.5), labels=(0, -1, 1)):
    """:343-374 -> cls (N, L) int64 in {-1, 0..K-1, K}, refine LTRB (N, L, 4), matches (N, L), matcher labels (N, L) int8, matched
    values (N, L).  Only matcher label 0 is rewritten to background (:357); an image without gt: cls = K (-1 outside), zero targets."""
    loc = torch.cat(ot.locations(level_hw, strides))
    xs, ys = loc[:, 0], loc[:, 1]
    out = [[] for _ in range(5)]
    for i, (b, c) in enumerate(zip(gt_boxes, gt_classes)):
        h, w = image_sizes[i]
        invalid = (xs >= w) | (ys >= h)
        b = b.float().reshape(-1, 4)
        cand = init_boxes[i].detach().float()
        if b.shape[0] == 0:
            cls = torch.full((len(xs),), num_classes, dtype=torch.int64)
            cls[invalid] = -1
            vals = [cls, torch.zeros(len(xs), 4), torch.zeros(len(xs), dtype=torch.int64), torch.full((len(xs),), labels[0], dtype=torch.int8), torch.zeros(len(xs))]
        else:
            q = od.pairwise_iou(b, cand)
            midx, mlab = od.matcher(q, list(thresholds), list(labels), True)
            cls = c[midx].clone().long()
            cls[mlab == 0] = num_classes
            cls[invalid] = -1
            m = b[midx]
            vals = [cls, torch.stack([xs - m[:, 0], ys - m[:, 1], m[:, 2] - xs, m[:, 3] - ys], dim=1), midx, mlab, q.max(dim=0)[0]]
        for o, v in zip(out, vals):
            o.append(v)
    return tuple(torch.stack(o) for o in out)


def rpd_losses(init_labels, init_reg, sel, refine_cls, refine_reg, logits, init_ltrb, refine_ltrb, ctr_logits, loc_strides, num_classes,
               alpha, gamma, iou_type, world=1):
    """:249-317 on flattened rows (M = N * L): init_labels / refine_cls (M,), init_reg / refine_reg (M, 4), sel (M,) bool, logits (M, K),
    init_ltrb / refine_ltrb (M, 4), ctr_logits (M,), loc_strides (M,).  With nothing selected ``reg_loss_init`` is 0 (the reference
    divides 0 by 0)."""
    K = num_classes
    ifg = (init_labels >= 0) & (init_labels != K)
    rfg = (refine_cls >= 0) & (refine_cls != K)
    n_init = max(int(ifg.sum()) / float(world), 1.0)
    n_ref = max(int(rfg.sum()) / float(world), 1.0)
    target = torch.zeros_like(logits)
    target[rfg, refine_cls[rfg]] = 1
    cls_loss = ol.sigmoid_focal_loss(logits, target, alpha, gamma, "sum") / n_ref            # no valid mask: cls = -1 rows are background
    score = slender_centerness(init_reg[ifg]).to(logits.dtype)
    score_sel = slender_centerness(init_reg[sel]).to(logits.dtype)
    if int(sel.sum()) > 0:
        reg_loss_init = ol.iou_loss_ltrb(init_ltrb[sel], init_reg[sel].to(logits.dtype), score_sel, iou_type) / (float(score_sel.sum()) / float(world))
    else:
        reg_loss_init = init_ltrb.sum() * 0
    norm = loc_strides[rfg].unsqueeze(-1) * 4
    reg_loss = ol.smooth_l1_loss(refine_ltrb[rfg] / norm, refine_reg[rfg].to(logits.dtype) / norm, 0.11, "sum") / max(1, n_ref)
    ctr_loss = F.binary_cross_entropy_with_logits(ctr_logits[ifg], score, reduction="sum") / n_init
    return {"cls_loss": cls_loss, "reg_loss_init": reg_loss_init, "reg_loss": reg_loss, "centerness_loss": ctr_loss}


def decode_ltrb(logits, ltrb, ctr, level_hw, strides, thresh, top_n):
    """One image, :428-462 per level: logits (L, K), ltrb (L, 4), ctr (L,) -> per level (boxes, scores, classes) in torch.nonzero()
    order, the top_n best by (score descending, (location, class) index ascending)."""
    loc = ot.locations(level_hw, strides)
    out, o = [], 0
    for l, (h, w) in enumerate(level_hw):
        sl = slice(o, o + h * w)
        o += h * w
        p = logits[sl].sigmoid()
        keep = p > thresh
        s = (p * ctr[sl].sigmoid()[:, None])[keep]
        nz = keep.nonzero()
        if s.numel() > top_n:
            pick = torch.sort(torch.sort(-s, stable=True).indices[:top_n]).values
            s, nz = s[pick], nz[pick]
        lo, d = loc[l][nz[:, 0]], ltrb[sl][nz[:, 0]]
        boxes = torch.stack([lo[:, 0] - d[:, 0], lo[:, 1] - d[:, 1], lo[:, 0] + d[:, 2], lo[:, 1] + d[:, 3]], dim=1)
        out.append((boxes, torch.sqrt(s), nz[:, 1]))
    return out


class OracleFCOSRepPoints(OracleFCOS):
    """Functional FCOSRepPoints over torch-layout CPU tensors: backbone, FPN and towers of OracleFCOS, the head of :641-707.  ``last``
    keeps the targets of the last call: init labels, selection, refine cls, matches, matched values (all (N, L))."""
    topk_per_box = 5

    @classmethod
    def from_hip_model(cls, model, emulate_bf16=False):
        o = super().from_hip_model(model, emulate_bf16)
        o.c.update(thresholds=list(model.iou_thresholds), labels=list(model.iou_labels), gmul=model.head.gradient_mul,
                   point_strides=list(model.head.point_strides))
        return o

    def head(self, feats):
        """-> logits (N, L, K), init / refine point offsets per level (N, 18, H, W), centerness logits (N, L)."""
        c = self.c
        K, n2 = c["num_classes"], 18
        base = torch.arange(-1, 2, dtype=torch.float32)
        base_off = torch.stack((base.repeat_interleave(3), base.repeat(3)), 1).reshape(1, -1, 1, 1).to(feats[0].dtype)      # y-major (:577-583)
        hook = (lambda s: self._act(s, "head")) if self.emu else None
        logits, oi_all, or_all, ctr_all = [], [], [], []
        for lvl, f in enumerate(feats):
            N = f.shape[0]
            ct, bt = self._tower("head.cls_tower", f), self._tower("head.bbox_tower", f)
            src = bt if c["ctr_on_reg"] else ct
            ctr = F.conv2d(src, self._wt(self.p["head.centerness.weight"])[:1], self.p["head.centerness.bias"][:1], padding=1)
            t = self._conv("head.offsets_init.0.conv", bt, 1, 1, relu=True)
            oi = F.conv2d(t, self._wt(self.p["head.offsets_init.1.conv.weight"])[:n2], self.p["head.offsets_init.1.conv.bias"][:n2])
            oi = oi * self.p["head.scales"][lvl]
            gm = (1 - c["gmul"]) * oi.detach() + c["gmul"] * oi
            off = gm.reshape(N, 9, 2, *gm.shape[-2:]).flip(2).reshape(N, n2, *gm.shape[-2:]) - base_off
            dc = self._act(_relu_at(deform_conv2d(ct, off, self._wt(self.p["head.deform_cls_conv.weight"]), None, 1, 1, 1, sample_hook=hook), "head.deform_cls_conv"), "head")
            dr = self._act(_relu_at(deform_conv2d(bt, off, self._wt(self.p["head.deform_reg_conv.weight"]), None, 1, 1, 1, sample_hook=hook), "head.deform_reg_conv"), "head")
            lg = F.conv2d(dc, self._wt(self.p["head.logits.weight"])[:K], self.p["head.logits.bias"][:K])
            orf = F.conv2d(dr, self._wt(self.p["head.offsets_refine.weight"])[:n2], self.p["head.offsets_refine.bias"][:n2]) + oi.detach()
            logits.append(lg.permute(0, 2, 3, 1).reshape(N, -1, K))
            ctr_all.append(ctr.permute(0, 2, 3, 1).reshape(N, -1))
            oi_all.append(oi)
            or_all.append(orf)
        return torch.cat(logits, 1), oi_all, or_all, torch.cat(ctr_all, 1)

    def losses(self, batched_inputs, world=1):
        c = self.c
        x = self.preprocess(batched_inputs)
        feats = self._fpn(self._bottom_up(x))
        level_hw = [tuple(f.shape[2:]) for f in feats]
        boxes = [b["instances"].gt_boxes.tensor.float().cpu() for b in batched_inputs]
        classes = [b["instances"].gt_classes.cpu() for b in batched_inputs]
        sizes = [tuple(b["image"].shape[-2:]) for b in batched_inputs]
        K = c["num_classes"]
        labels, reg_t, _score, _idx, sel = slender_targets(level_hw, c["strides"], boxes, classes, c["radius"], K, self.topk_per_box)
        logits, oi, orf, ctr = self.head(feats)
        init_ltrb = ltrb_rows(offsets2ltrb(oi, c["point_strides"]))
        refine_ltrb = ltrb_rows(offsets2ltrb(orf, c["point_strides"]))
        init_boxes = decode_boxes(init_ltrb.detach().float(), level_hw, c["strides"])
        rcls, rreg, matches, mlab, vals = refine_targets(level_hw, c["strides"], init_boxes, boxes, classes, sizes, K, c["thresholds"], c["labels"])
        self.last = dict(labels=labels, sel=sel, cls=rcls, matches=matches, vals=vals, mlab=mlab)
        N = logits.shape[0]
        st = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(level_hw, c["strides"])]).repeat(N).to(logits.dtype)
        return rpd_losses(labels.reshape(-1), reg_t.reshape(-1, 4), sel.reshape(-1), rcls.reshape(-1), rreg.reshape(-1, 4),
                          logits.reshape(-1, K), init_ltrb.reshape(-1, 4), refine_ltrb.reshape(-1, 4), ctr.reshape(-1), st, K,
                          c["alpha"], c["gamma"], c["iou_type"], world)
