#!/usr/bin/env python
"""Generates the golden vectors of FCOSRepPoints under tests/golden/fcos_reppoints/ by running the REFERENCE's own Python (read-only)
on synthetic cases.  Runs only where the reference checkout of tests/golden/make_golden.py exists; nothing from the reference is
copied: only inputs / outputs (numpy arrays) and meta.json are written.

The reference file slender_det/modeling/meta_arch/fcos/fcos_rpd_s1_topk.py is loaded with importlib under the stub modules of
tests/golden/make_golden.py and make_golden_reppoints.py (whose Boxes container and restated third-party operators are reused):
    compute_centerness_targets (:25-54), compute_targets_for_locations (:57-134)      pure reference Python
    FCOSRepPoints.get_ground_truth (:320-376)           reference Python x restated detectron2 pairwise_iou / Matcher
    FCOSRepPointsHead.offsets2ltrb (:709-745)           pure reference Python
    FCOSRepPoints.losses (:249-317)                     reference Python x restated fvcore focal / smooth-L1
detectron2 / fvcore are not installed; what passes through a restated operator is labelled so in meta.json.

Conditions on the INPUTS that the generator asserts and records (they make the reference's result unambiguous; they are no bars):
  * ``torch.topk(sorted=False)`` (:119) leaves ties at the cut open: for every gt box with more than 5 positives the 5th and 6th
    largest slender score differ by at least 1e-3 relative;
  * in the ``iou`` loss fixture every selected row has all four predicted and target distances > 0 (no logarithm sees a non-positive
    number); the ``giou`` fixture deliberately contains selected rows with a negative predicted distance;
  * no candidate IoU lies within 1e-4 of a matcher threshold, and no gt's best IoU is attained twice within 1e-6 relative.

    python tests/golden/fcos_reppoints/make_golden_fcos_reppoints.py
"""
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(OUT)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(GOLDEN, "fcos_topk"))

import make_golden as MG  # noqa: E402  (REF, _load, _stub, install_stubs, focal_restated)
import make_golden_reppoints as MR  # noqa: E402  (Boxes, pairwise_iou, Matcher, smooth_l1_restated)
from make_golden_fcos_topk import IMG_H, IMG_W, LEVEL_HW, STRIDES, random_gts  # noqa: E402
from oracle import fcos_targets as ot  # noqa: E402

TOPK = 5
MIN_GAP = 1e-3
THRESHOLDS, LABELS = [0.4, 0.5], [0, -1, 1]
POINT_STRIDES = [1, 2, 4, 8, 16]


def load_reference():
    MG.install_stubs()
    iou_mod = MG._load("ref_iou_loss", "slender_det/layers/iou_loss.py")
    scale_mod = MG._load("ref_scale", "slender_det/layers/scale.py")
    utils = MG._load("ref_fcos_utils", "slender_det/modeling/meta_arch/fcos/utils.py")
    MG._stub("fvcore.nn", sigmoid_focal_loss_jit=MG.focal_restated, smooth_l1_loss=MR.smooth_l1_restated)
    MG._stub("detectron2.structures", ImageList=None, Instances=None, Boxes=MR.Boxes, pairwise_iou=MR.pairwise_iou)
    MG._stub("detectron2.modeling.matcher", Matcher=MR.Matcher)
    MG._stub("detectron2.layers", cat=lambda ts, dim=0: ts[0] if len(ts) == 1 else torch.cat(ts, dim), ShapeSpec=SimpleNamespace, batched_nms=None,
             DeformConv=None, ModulatedDeformConv=None)
    MG._stub("slender_det")
    MG._stub("slender_det.modeling")
    MG._stub("slender_det.modeling.backbone", build_backbone=None)
    MG._stub("slender_det.layers", Scale=scale_mod.Scale, iou_loss=iou_mod.iou_loss, DFConv2d=None)
    MG._stub("refpkg")
    sys.modules["refpkg.utils"] = utils
    spec = importlib.util.spec_from_file_location("refpkg.fcos_rpd_s1_topk", os.path.join(MG.REF, "slender_det/modeling/meta_arch/fcos/fcos_rpd_s1_topk.py"))
    rp = importlib.util.module_from_spec(spec)
    sys.modules["refpkg.fcos_rpd_s1_topk"] = rp
    spec.loader.exec_module(rp)
    return utils, rp


def inst(b, c, size=(IMG_H, IMG_W)):
    return SimpleNamespace(gt_boxes=MR.Boxes(b), gt_classes=c, image_size=size)


def sizes_of_interest(locs):
    soi = [[-1, 64], [64, 128], [128, 256], [256, 512], [512, 100000000]]
    return torch.cat([torch.tensor(soi[l], dtype=torch.float32)[None].expand(len(p), -1) for l, p in enumerate(locs)], dim=0)


def reference_targets(utils, rp, boxes, classes, radius, num_classes):
    locs = utils.compute_locations(LEVEL_HW, STRIDES, torch.device("cpu"))
    labels, reg, topk = rp.compute_targets_for_locations(locs, [inst(b, c.clone()) for b, c in zip(boxes, classes)], sizes_of_interest(locs),
                                                         STRIDES, radius, num_classes)
    return locs, labels, reg, topk


def cut_gaps(rp, locs, boxes, classes, labels, reg, radius, num_classes):
    """Relative gap between the 5th and 6th largest slender score of every gt with more than 5 positives; the largest relative error of
    the reference's float32 score against float64; checks that the oracle's arg-min indices reproduce the reference's targets."""
    pts = [len(l) for l in locs]
    allp = torch.cat(locs)
    gaps, many, err = [], 0, 0.0
    for i, (b, c) in enumerate(zip(boxes, classes)):
        lab, rt, idx = ot.targets_for_image(allp, pts, STRIDES, b, c, radius, num_classes, return_inds=True)
        assert torch.equal(lab, labels[i]) and torch.equal(rt, reg[i])
        fg = (lab >= 0) & (lab != num_classes)
        if int(fg.sum()):
            s32, s64 = rp.compute_centerness_targets(rt[fg]), rp.compute_centerness_targets(rt[fg].double())
            err = max(err, float(((s32.double() - s64).abs() / s64).max()))
        for g in range(b.shape[0]):
            rows = fg & (idx == g)
            if int(rows.sum()) > TOPK:
                many += 1
                s = rp.compute_centerness_targets(rt[rows]).sort(descending=True).values
                gaps.append(float((s[TOPK - 1] - s[TOPK]) / s[TOPK - 1]))
    return gaps, many, err


def candidate_boxes(g, n_images, lo=0.5, hi=4.0):
    """Init boxes around every location: LTRB distances of lo..hi strides."""
    locs = torch.cat(ot.locations(LEVEL_HW, STRIDES))
    st = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(LEVEL_HW, STRIDES)])
    d = (torch.rand(n_images, len(locs), 4, generator=g) * (hi - lo) + lo) * st[None, :, None]
    return torch.stack([locs[None, :, 0] - d[..., 0], locs[None, :, 1] - d[..., 1], locs[None, :, 0] + d[..., 2], locs[None, :, 1] + d[..., 3]], dim=2)


def matcher_margins(boxes, cand):
    """(smallest |IoU - threshold| over all pairs, smallest relative gap between the two largest IoUs of a gt) over the batch."""
    thr, tie = 1.0, 1.0
    for b, c in zip(boxes, cand):
        q = MR.pairwise_iou(MR.Boxes(b), MR.Boxes(c))
        for t in THRESHOLDS:
            thr = min(thr, float((q - t).abs().min()))
        top = q.topk(2, dim=1).values
        assert bool((top[:, 0] > 0).all()), "a gt box without any overlapping candidate"
        tie = min(tie, float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
    return thr, tie


def points_for(g, ltrb_rows, negative_rows=None):
    """Nine (x, y) points per location, in units of the level's point stride, whose min / max give the LTRB rows (N, L, 4): point 0 is
    (-l, -t), point 1 is (r, b), the other seven lie strictly between.  Returned per level as (N, 18, H, W)."""
    N, L = ltrb_rows.shape[:2]
    ps = torch.cat([torch.full((h * w,), float(p)) for (h, w), p in zip(LEVEL_HW, POINT_STRIDES)])
    d = ltrb_rows / ps[None, :, None]
    u = torch.rand(N, L, 9, 2, generator=g) * 0.8 + 0.1
    lo = torch.stack((-d[..., 0], -d[..., 1]), dim=-1)[:, :, None]
    hi = torch.stack((d[..., 2], d[..., 3]), dim=-1)[:, :, None]
    pts = lo + (hi - lo) * u
    pts[:, :, 0], pts[:, :, 1] = lo[:, :, 0], hi[:, :, 0]
    perm = torch.stack([torch.randperm(9, generator=g) for _ in range(N * L)]).view(N, L, 9)      # the extrema sit at any index
    pts = torch.gather(pts, 2, perm[..., None].expand(-1, -1, -1, 2))
    rows = pts.reshape(N, L, 18)
    out, o = [], 0
    for h, w in LEVEL_HW:
        out.append(rows[:, o:o + h * w].reshape(N, h, w, 18).permute(0, 3, 1, 2).contiguous())
        o += h * w
    return out


def main():
    assert os.path.isdir(MG.REF), "make_golden_fcos_reppoints.py only runs where the reference checkout exists"
    utils, rp = load_reference()
    meta = {"restated_operators": {"sigmoid_focal_loss_jit": "make_golden.py focal_restated", "smooth_l1_loss": "make_golden_reppoints.py smooth_l1_restated",
                                   "Matcher": "make_golden_reppoints.py Matcher", "pairwise_iou": "make_golden_reppoints.py pairwise_iou"}}
    score_err = 0.0

    # ---------------------------------------------------------------- (a) targets: two seeds x two radii, pure reference
    def clears(seed):
        boxes, classes = random_gts(seed)
        for radius in (1.5, 0.0):
            locs, labels, reg, _ = reference_targets(utils, rp, boxes, classes, radius, 80)
            gaps, many, _ = cut_gaps(rp, locs, boxes, classes, labels, reg, radius, 80)
            if many < 2 or min(gaps) < MIN_GAP:
                return False
        return True

    clearing = [s for s in range(16) if clears(s)]
    seeds = clearing[:2]
    assert len(seeds) == 2, clearing
    min_gap, kept = 1.0, {}
    for seed in seeds:
        boxes, classes = random_gts(seed)
        out = {"level_hw": np.array(LEVEL_HW), "strides": np.array(STRIDES), "num_classes": np.array(80)}
        for i, (b, c) in enumerate(zip(boxes, classes)):
            out[f"boxes{i}"], out[f"classes{i}"] = b.numpy(), c.numpy()
        for radius in (1.5, 0.0):
            locs, labels, reg, topk = reference_targets(utils, rp, boxes, classes, radius, 80)
            gaps, many, err = cut_gaps(rp, locs, boxes, classes, labels, reg, radius, 80)
            assert many >= 2 and min(gaps) >= MIN_GAP, (seed, radius, many, gaps)
            min_gap, score_err = min(min_gap, min(gaps)), max(score_err, err)
            fg = labels != 80
            score = torch.zeros(labels.shape)
            score[fg] = rp.compute_centerness_targets(reg[fg])
            out[f"gt_classes_r{radius}"], out[f"reg_targets_r{radius}"] = labels.numpy(), reg.numpy()
            out[f"topk_locations_r{radius}"], out[f"scores_r{radius}"] = topk.numpy(), score.numpy()
            out[f"num_gt_over_topk_r{radius}"] = np.array(many)
        np.savez_compressed(os.path.join(OUT, f"targets_seed{seed}.npz"), **out)
        kept[seed] = (boxes, classes)
        meta[f"targets_seed{seed}.npz"] = ("reference: fcos_rpd_s1_topk.py:25-134 (compute_targets_for_locations, compute_centerness_targets), pure "
                                           "reference Python; 3 images, 128 x 160, radius 1.5 and 0")

    # ---------------------------------------------------------------- (b) get_ground_truth on given init boxes
    K = 80
    boxes, classes = kept[seeds[0]]
    sizes = [(IMG_H, IMG_W), (IMG_H, IMG_W - 28), (IMG_H - 20, IMG_W)]      # image 1: the last columns, image 2: the last rows of locations lie outside
    g = torch.Generator().manual_seed(200)
    cand = candidate_boxes(g, len(boxes))
    thr, tie = matcher_margins(boxes, cand)
    assert thr >= 1e-4 and tie >= 1e-6, (thr, tie)
    locs = utils.compute_locations(LEVEL_HW, STRIDES, torch.device("cpu"))
    self_ns = SimpleNamespace(fpn_strides=STRIDES, center_sampling_radius=1.5, num_classes=K, bbox_matcher=MR.Matcher(THRESHOLDS, LABELS, True))
    gts = [inst(b, c.clone(), s) for b, c, s in zip(boxes, classes, sizes)]
    ic, ir, rc, rr, tk = rp.FCOSRepPoints.get_ground_truth(self_ns, locs, cand, gts)
    assert int((rc == -1).sum()) > 0 and int(((rc >= 0) & (rc != K)).sum()) > len(torch.cat(boxes))
    out = {"level_hw": np.array(LEVEL_HW), "strides": np.array(STRIDES), "num_classes": np.array(K), "radius": np.array(1.5),
           "image_sizes": np.array(sizes), "thresholds": np.array(THRESHOLDS), "labels": np.array(LABELS), "init_boxes": cand.numpy(),
           "init_gt_classes": ic.numpy(), "init_reg_targets": ir.numpy(), "refine_gt_classes": rc.numpy(), "refine_reg_targets": rr.numpy(),
           "topk_locations": tk.numpy()}
    for i, (b, c) in enumerate(zip(boxes, classes)):
        out[f"boxes{i}"], out[f"classes{i}"] = b.numpy(), c.numpy()
    np.savez_compressed(os.path.join(OUT, "ground_truth.npz"), **out)
    meta["ground_truth.npz"] = ("reference-Python x restated-op: FCOSRepPoints.get_ground_truth (fcos_rpd_s1_topk.py:320-376) with detectron2 pairwise_iou / "
                                "Matcher restated; 3 images of 128x160, 128x132, 108x160 in a 128 x 160 batch, random init boxes of 0.5-4 strides")
    meta["ground_truth_min_abs_iou_minus_threshold"], meta["ground_truth_min_relative_gap_of_a_gt_best_iou"] = thr, tie

    # ---------------------------------------------------------------- (c) offsets2ltrb on random points, pure reference
    g = torch.Generator().manual_seed(300)
    deltas = [torch.randn(2, 18, h, w, generator=g) * 3 for h, w in LEVEL_HW]
    ltrb = rp.FCOSRepPointsHead.offsets2ltrb(None, deltas)
    out = {"level_hw": np.array(LEVEL_HW)}
    for l in range(len(LEVEL_HW)):
        out[f"points{l}"], out[f"ltrb{l}"] = deltas[l].numpy(), ltrb[l].numpy()
    np.savez_compressed(os.path.join(OUT, "offsets2ltrb.npz"), **out)
    meta["offsets2ltrb.npz"] = "reference: FCOSRepPointsHead.offsets2ltrb (fcos_rpd_s1_topk.py:709-745), pure reference Python; N = 2, random points"

    # ---------------------------------------------------------------- (d) losses: N = 2, 8 classes
    K = 8
    boxes, classes = kept[seeds[0]]
    boxes, classes = boxes[:2], [c % K for c in classes[:2]]
    sizes = [(IMG_H, IMG_W), (IMG_H, IMG_W - 28)]
    st_rows = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(LEVEL_HW, STRIDES)])
    for radius, iou_type in ((1.5, "giou"), (0.0, "iou")):
        g = torch.Generator().manual_seed(400 + int(radius))
        locs, labels, reg, topk = reference_targets(utils, rp, boxes, classes, radius, K)
        gaps, many, err = cut_gaps(rp, locs, boxes, classes, labels, reg, radius, K)
        assert many >= 1 and min(gaps) >= MIN_GAP, (radius, many, gaps)
        min_gap, score_err = min(min_gap, min(gaps)), max(score_err, err)
        # predicted init distances: near the stage-1 target on foreground rows (so that the IoU matcher finds real positives), 0.5-4
        # strides elsewhere; the refine distances are the init ones times 0.8-1.2
        fg = labels != K
        d_init = (torch.rand(2, len(st_rows), 4, generator=g) * 3.5 + 0.5) * st_rows[None, :, None]
        d_init[fg] = reg[fg] * (torch.rand(int(fg.sum()), 4, generator=g) * 0.8 + 0.6)
        if iou_type == "giou":          # a negative left / top distance on every third selected row: the nine points lie right of / below the location
            rows = topk.nonzero()[::3]
            d_init[rows[:, 0], rows[:, 1], 0] *= -0.25
            d_init[rows[1::2, 0], rows[1::2, 1], 1] *= -0.25
            assert bool((d_init[topk] < 0).any())
        else:
            assert bool((d_init[topk] > 0).all()) and bool((reg[topk] > 0).all())
        d_ref = d_init * (torch.rand(d_init.shape, generator=g) * 0.4 + 0.8)
        pts_init, pts_ref = points_for(g, d_init), points_for(g, d_ref)
        logits = [torch.randn(2, K, h, w, generator=g) * 2 - 2 for h, w in LEVEL_HW]
        ctrness = [torch.randn(2, 1, h, w, generator=g) for h, w in LEVEL_HW]
        preds = [[t.clone().requires_grad_(True) for t in ts] for ts in (logits, pts_init, pts_ref, ctrness)]
        box_init = rp.FCOSRepPointsHead.offsets2ltrb(None, preds[1])
        box_ref = rp.FCOSRepPointsHead.offsets2ltrb(None, preds[2])
        rows_init = torch.cat([utils.permute_to_N_HW_K(x, 4) for x in box_init], dim=1).detach()
        allp = torch.cat(locs)
        init_boxes = torch.stack([allp[None, :, 0] - rows_init[..., 0], allp[None, :, 1] - rows_init[..., 1],
                                  allp[None, :, 0] + rows_init[..., 2], allp[None, :, 1] + rows_init[..., 3]], dim=2)      # :229-232
        thr, tie = matcher_margins(boxes, init_boxes)
        assert thr >= 1e-4 and tie >= 1e-6, (iou_type, thr, tie)
        self_ns = SimpleNamespace(fpn_strides=STRIDES, center_sampling_radius=radius, num_classes=K, bbox_matcher=MR.Matcher(THRESHOLDS, LABELS, True),
                                  focal_loss_alpha=0.25, focal_loss_gamma=2.0, iou_loss_type=iou_type)
        gts = [inst(b, c.clone(), s) for b, c, s in zip(boxes, classes, sizes)]
        ic, ir, rc, rr, tk = rp.FCOSRepPoints.get_ground_truth(self_ns, locs, init_boxes, gts)
        assert torch.equal(tk, topk) and torch.equal(ic, labels)
        n_ref = int(((rc >= 0) & (rc != K)).sum())
        assert n_ref > len(torch.cat(boxes)), n_ref
        losses = rp.FCOSRepPoints.losses(self_ns, ic, ir, rc, rr, preds[0], box_init, box_ref, preds[3], st_rows, tk)
        flat = preds[0] + preds[1] + preds[2] + preds[3]
        grads = torch.autograd.grad(sum(losses.values()), flat)
        n = len(LEVEL_HW)
        out = {"level_hw": np.array(LEVEL_HW), "strides": np.array(STRIDES), "num_classes": np.array(K), "radius": np.array(radius),
               "alpha": np.array(0.25), "gamma": np.array(2.0), "image_sizes": np.array(sizes), "thresholds": np.array(THRESHOLDS),
               "labels": np.array(LABELS), "init_gt_classes": ic.numpy(), "init_reg_targets": ir.numpy(), "topk_locations": tk.numpy(),
               "refine_gt_classes": rc.numpy(), "refine_reg_targets": rr.numpy(), "num_refine_positives": np.array(n_ref)}
        for i, (b, c) in enumerate(zip(boxes, classes)):
            out[f"boxes{i}"], out[f"classes{i}"] = b.numpy(), c.numpy()
        for l in range(n):
            for j, k in enumerate(("logits", "points_init", "points_refine", "ctrness")):
                out[f"{k}{l}"], out[f"grad_{k}{l}"] = flat[j * n + l].detach().numpy(), grads[j * n + l].numpy()
        out.update({"loss::" + k: v.detach().numpy() for k, v in losses.items()})
        np.savez_compressed(os.path.join(OUT, f"losses_{iou_type}.npz"), **out)
        meta[f"losses_{iou_type}.npz"] = ("reference-Python x restated-op: offsets2ltrb + FCOSRepPoints.get_ground_truth + FCOSRepPoints.losses "
                                          "(fcos_rpd_s1_topk.py:249-376, :709-745) with focal / smooth-L1 / Matcher / pairwise_iou restated; N = 2, 8 classes, "
                                          f"radius {radius}, {iou_type}; losses and autograd gradients of their sum w.r.t. logits, both point sets and centerness")
        meta[f"losses_{iou_type}_min_abs_iou_minus_threshold"], meta[f"losses_{iou_type}_min_relative_gap_of_a_gt_best_iou"] = thr, tie
    meta["seeds"], meta["seeds_clearing_the_gap_of_0_to_15"] = seeds, clearing
    meta["min_relative_gap_5th_6th_slender_score"] = min_gap
    meta["max_relative_error_of_float32_slender_score_vs_float64"] = score_err
    json.dump(meta, open(os.path.join(OUT, "meta.json"), "w"), indent=1, sort_keys=True)
    print("wrote", sorted(k for k in meta if k.endswith(".npz")), "seeds", seeds, "of", clearing, "min gap", min_gap, "score err", score_err)


if __name__ == "__main__":
    main()
