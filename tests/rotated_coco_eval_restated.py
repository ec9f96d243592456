"""Plain numpy restatement of the rotated-box COCO evaluation - detectron2's RotatedCOCOeval / RotatedCOCOEvaluator over
pycocotools' COCOeval - as the package documents it (test infrastructure, no HIP).

    restated_inputs       gts / dets in the flat form below, from a COCO json dict and the prediction arrays
    match_segment         COCOeval.evaluateImg for one (image, category) on a given float32 IoU matrix
    match_and_accumulate  evaluate + accumulate; the IoUs come from ``iou_fn(dt_boxes [D, 5], gt_boxes [G, 5]) -> [D, G] float32``
    summarize_area        pycocotools' 12 stats
    derive_results        {"AP", "AP50", "AP75", "APs", "APm", "APl"[, "AP-<name>"]}
    derive_ratio_results  the 16 ratio-bucketed stats by name (the package's slenderness extension)

  gts   list of dicts with image_id, category_id (dataset id), box5 float32 [5], iscrowd, val (float64: area or ratio), json order;
  dets  dict of numpy arrays image_id, category_id (dataset id), box5 [N, 5] float32, score float32, val [N] float64.
"""
import numpy as np
import torch

import coco_eval_restated as RS

IOU_THRS, REC_THRS, MAX_DETS, RATIO_RNG = RS.IOU_THRS, RS.REC_THRS, RS.MAX_DETS, RS.RATIO_RNG
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
RATIO_LBL = ["all", " 0  - 1/5", "1/5 - 1/3", "1/3 - 3", "3/1 - 5/1", "5/1 - INF"]


def oracle_iou(dt, gt):
    """pairwise_iou_rotated(dt, gt) on the CPU (python loops: a few hundred pairs at most)."""
    from oracle.detection import pairwise_iou_rotated

    return pairwise_iou_rotated(torch.from_numpy(np.ascontiguousarray(dt)), torch.from_numpy(np.ascontiguousarray(gt))).numpy()


def gt_box5(bbox):
    """A five-number bbox as it is; XYWH -> (x + w/2, y + h/2, w, h, 0), computed in float32 on the float32-rounded json numbers."""
    b = np.array(bbox, np.float32)
    if len(b) == 5:
        return b
    two = np.float32(2)
    return np.array([b[0] + b[2] / two, b[1] + b[3] / two, b[2], b[3], np.float32(0)], np.float32)


def pred_box5(boxes):
    """[N, 5] as it is; [N, 4] XYXY -> XYWH -> centre form, float32 throughout."""
    b = np.asarray(boxes, np.float32)
    if b.shape[1] == 5:
        return b
    wh = b[:, 2:] - b[:, :2]
    return np.concatenate([b[:, :2] + wh / np.float32(2), wh, np.zeros((len(b), 1), np.float32)], axis=1).astype(np.float32)


def restated_inputs(dataset, preds, bucket="area"):
    """(img_ids, cat_ids sorted, gts, dets).  bucket "area": gt val = "area" or w * h, dt val = w * h; "ratio": gt val = "ratio"
    or min(w, h) / max(w, h), dt val = w / h (float64 of the float32 box)."""
    img_ids = sorted(im["id"] for im in dataset["images"])
    cat_ids = sorted(c["id"] for c in dataset["categories"])
    gts = []
    for a in dataset.get("annotations", []):
        w, h = float(a["bbox"][2]), float(a["bbox"][3])
        if bucket == "area":
            val = float(a["area"]) if "area" in a else w * h
        else:
            val = float(a["ratio"]) if "ratio" in a else (min(w, h) / max(w, h) if max(w, h) > 0 else 0.0)
        gts.append({"image_id": a["image_id"], "category_id": a["category_id"], "box5": gt_box5(a["bbox"]),
                    "iscrowd": int(bool(a.get("iscrowd", 0) or a.get("ignore", 0))), "val": val, "id": a["id"]})
    b = pred_box5(preds["boxes"]) if len(preds["boxes"]) else np.zeros((0, 5), np.float32)
    w64, h64 = b[:, 2].astype(np.float64), b[:, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        val = w64 * h64 if bucket == "area" else w64 / h64
    dets = {"image_id": np.asarray(preds["image_id"], np.int64),
            "category_id": np.array([cat_ids[c] for c in preds["category"]], np.int64), "box5": b,
            "score": np.asarray(preds["score"], np.float32), "val": val}
    return img_ids, cat_ids, gts, dets


def match_segment(ious, gt_crowd, gt_val, dt_val, ranges):
    """One (image, category) whose detections are already in stable descending score order and cut to maxDets[-1].  ious [D, G]
    float32 (None when D or G is 0).  Returns matched [T, A, D] bool, ignored [T, A, D] bool, npig [A].  The scan compares in
    float32: torch compares a float32 element with a float64 scalar in float32."""
    T, A = len(IOU_THRS), len(ranges)
    G, D = len(gt_val), len(dt_val)
    matched = np.zeros((T, A, D), bool)
    ignored = np.zeros((T, A, D), bool)
    npig = np.zeros(A, np.int64)
    if ious is not None:
        ious = np.asarray(ious, np.float32)
        assert ious.shape == (D, G)
    for a, (lo, hi) in enumerate(ranges):
        ig = np.array([bool(gt_crowd[j]) or gt_val[j] < lo or gt_val[j] > hi for j in range(G)], bool)
        npig[a] = int((~ig).sum())
        perm = [j for j in range(G) if not ig[j]] + [j for j in range(G) if ig[j]]      # ignored gts last, each half in its own order
        for t, thr in enumerate(IOU_THRS):
            taken = np.zeros(G, bool)
            for i in range(D if ious is not None else 0):
                best, m = np.float32(min(thr, 1 - 1e-10)), -1
                for j in perm:
                    if taken[j] and not gt_crowd[j]:
                        continue
                    if m > -1 and not ig[m] and ig[j]:
                        break
                    if ious[i, j] < best:
                        continue
                    best, m = ious[i, j], j
                if m == -1:
                    continue
                matched[t, a, i] = True
                ignored[t, a, i] = ig[m]
                taken[m] = True
        for i in range(D):
            if dt_val[i] < lo or dt_val[i] > hi:
                ignored[:, a, i] |= ~matched[:, a, i]
    return matched, ignored, npig


def match_and_accumulate(img_ids, cat_ids, gts, dets, ranges, iou_fn=oracle_iou):
    """precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M] (float64, -1 where a category has no gt in the
    range).  Matching once with maxDets[-1]; accumulate takes the first maxDets[m] of each segment."""
    img_ids, cat_ids = sorted(img_ids), sorted(cat_ids)
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(ranges), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    gseg, dseg = {}, {}
    for gt in gts:
        gseg.setdefault((gt["image_id"], gt["category_id"]), []).append(gt)
    for n in range(len(dets["score"])):
        dseg.setdefault((int(dets["image_id"][n]), int(dets["category_id"][n])), []).append(n)
    for k, cat in enumerate(cat_ids):
        per_img = []
        for img in img_ids:
            g = gseg.get((img, cat), [])
            dn = np.array(dseg.get((img, cat), []), np.int64)
            if not g and not len(dn):
                continue
            sc = dets["score"][dn].astype(np.float64)
            order = RS._stable_desc(sc)[:MAX_DETS[-1]]
            dn = dn[order]
            ious = None
            if len(g) and len(dn):
                ious = iou_fn(dets["box5"][dn], np.stack([x["box5"] for x in g]))      # detection first, gt second
            mt, ig, npig = match_segment(ious, [x["iscrowd"] for x in g], [x["val"] for x in g], dets["val"][dn], ranges)
            per_img.append((sc[order], mt, ig, npig))
        if not per_img:
            continue
        for a in range(A):
            npig = int(sum(p[3][a] for p in per_img))
            if npig == 0:
                continue
            for m, md in enumerate(MAX_DETS):
                sc = np.concatenate([p[0][:md] for p in per_img])
                inds = RS._stable_desc(sc)
                mt = np.concatenate([p[1][:, a, :md] for p in per_img], axis=1)[:, inds]
                ig = np.concatenate([p[2][:, a, :md] for p in per_img], axis=1)[:, inds]
                sc = sc[inds]
                tp = np.cumsum(mt & ~ig, axis=1).astype(np.float64)
                fp = np.cumsum(~mt & ~ig, axis=1).astype(np.float64)
                nd = tp.shape[1]
                for t in range(T):
                    rc = tp[t] / npig
                    pr = tp[t] / (fp[t] + tp[t] + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr
                    pos = np.searchsorted(rc, REC_THRS, side="left")
                    ok = pos < nd
                    q = np.zeros(R)
                    s = np.zeros(R)
                    q[ok] = pr[pos[ok]]
                    s[ok] = sc[pos[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = s
    return precision, recall, scores


def summarize_area(precision, recall):
    """AP, AP@.5, AP@.75, AP small / medium / large (100), AR@1, AR@10, AR@100, AR small / medium / large (100): the mean over the
    entries > -1, or -1 when there are none."""
    def one(ap, t=None, a=0, m=2):
        s = precision if ap else recall
        if t is not None:
            s = s[np.where(t == IOU_THRS)[0]]
        s = s[:, :, :, [a], [m]] if ap else s[:, :, [a], [m]]
        v = s[s > -1]
        return -1 if len(v) == 0 else np.mean(v)

    out = [one(1), one(1, .5), one(1, .75)] + [one(1, a=a) for a in range(1, 4)]
    out += [one(0, m=0), one(0, m=1), one(0, m=2)] + [one(0, a=a) for a in range(1, 4)]
    return np.array(out)


def derive_results(stats, precision, class_names):
    names = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    if stats is None:
        return {n: float("nan") for n in names}
    res = {}
    for i, name in enumerate(names):
        res[name] = float(stats[i] * 100 if stats[i] >= 0 else "nan")
    if class_names is None or len(class_names) <= 1:
        return res
    for k, n in enumerate(class_names):
        p = precision[:, :, k, 0, -1]
        p = p[p > -1]
        res["AP-" + n] = float(np.mean(p) * 100) if p.size else float("nan")
    return res


def derive_ratio_results(stats):
    keys = ["AP", "AP50", "AP75"] + ["AP-" + lbl for lbl in RATIO_LBL[1:]] + ["AR@1", "AR@10", "AR@100"] + ["AR-" + lbl for lbl in RATIO_LBL[1:]]
    if stats is None:
        return {k: float("nan") for k in keys}
    return {k: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, k in enumerate(keys)}
