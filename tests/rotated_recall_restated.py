"""Plain numpy / torch restatement of the slenderness-bucketed recall pass on rotated boxes (test infrastructure, no HIP): the loop of
coco_eval_restated.proposal_ar - _evaluate_predictions_ar, slender_det/evaluation/coco_evaluation.py:283-417 - on five-number boxes.

    proposal_ar_rotated   the rounds; the overlaps come from ``iou_fn(dt [D, 5], gt [G, 5]) -> [D, G]`` float32, a gt's area is the
                          float32 product w * h of its box, its ratio the annotation's ``ratio``

  images        list of (image_id, boxes5 float32 [D, 5] (cx, cy, w, h, angle_deg), contiguous classes [D]) in prediction order;
  gts_by_image  {image_id: [dict with box5 (five float32), category_id (dataset id), ratio, iscrowd], ...} in json order.
"""
import numpy as np
import torch

from coco_eval_restated import AR_AREAS, AR_RATIOS, _in, ar_results  # noqa: F401 - ar_results is part of this module's surface


def proposal_ar_rotated(images, gts_by_image, cat_to_contig, num_cats, iou_fn, limit=100):
    """Returns recalls [T, K+1, R, A] float32, ar, mar (0-dim float32), num_pos [K+1, R, A] int64, the number of images that took
    part and hits [T, K+1, R, A] int64.  Each image keeps its first `limit` boxes AND classes."""
    K, R, A = num_cats + 1, len(AR_RATIOS), len(AR_AREAS)
    thr = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)
    T = len(thr)
    hit = torch.zeros((T, K, R, A), dtype=torch.float32)
    num_pos = torch.zeros((K, R, A), dtype=torch.int64)
    used = 0
    for image_id, boxes, classes in images:
        anno = [o for o in gts_by_image.get(image_id, []) if o["iscrowd"] == 0]
        if len(anno) == 0 or len(boxes) == 0:
            continue
        used += 1
        boxes, classes = boxes[:limit], classes[:limit]
        pb = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 5))
        gb = np.ascontiguousarray(np.stack([np.asarray(o["box5"], np.float32) for o in anno]))
        gc = [cat_to_contig[o["category_id"]] for o in anno]
        gr = torch.tensor([o["ratio"] for o in anno], dtype=torch.float32)
        ga = torch.from_numpy(gb[:, 2] * gb[:, 3])                     # float32 product
        rs = [[r for r, (lo, hi) in enumerate(AR_RATIOS) if _in(gr[j], lo, hi)] for j in range(len(anno))]
        as_ = [[a for a, (lo, hi) in enumerate(AR_AREAS) if _in(ga[j], lo, hi)] for j in range(len(anno))]
        for j in range(len(anno)):
            for r in rs[j]:
                for a in as_[j]:
                    num_pos[gc[j], r, a] += 1
                    num_pos[K - 1, r, a] += 1
        ov = torch.from_numpy(np.array(iou_fn(pb, gb), np.float32, copy=True))
        assert ov.shape == (len(pb), len(gb))
        same = torch.tensor([[int(c) == g for g in gc] for c in classes], dtype=torch.bool)
        ovm = ov * same
        img_hit = torch.zeros((T, K, R, A), dtype=torch.float32)
        for _ in range(min(len(pb), len(anno))):
            colmax, rowarg = ov.max(dim=0)
            best, gi = colmax.max(dim=0)
            colmax_m, rowarg_m = ovm.max(dim=0)
            best_m, gi_m = colmax_m.max(dim=0)
            k = gc[int(gi_m)]
            for r in rs[int(gi_m)]:
                for a in as_[int(gi_m)]:
                    img_hit[:, k, r, a] += (best_m >= thr).float()
                    img_hit[:, K - 1, r, a] += (best >= thr).float()
            ov[rowarg[gi], :] = -1
            ov[:, gi] = -1
            ovm[rowarg_m[gi_m], :] = -1
            ovm[:, gi_m] = -1
        hit += img_hit
    cnt = num_pos.float()
    recalls = hit / torch.max(cnt, torch.tensor(1).float())
    ar = recalls[:, -1, 0, 0].mean()
    mar = recalls[:, :-1, 0, 0].mean()
    return recalls, ar, mar, num_pos, used, hit.to(torch.int64)
