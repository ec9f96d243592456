"""Plain numpy / torch restatement of the three passes of the slender-object COCO evaluation (test infrastructure, no HIP).

    match_and_accumulate  COCOeval.evaluate + accumulate (slender_det/evaluation/cocoeval.py:123-432) for bbox, ratio-bucketed
    summarize             COCOeval.summarize's 16 stats (cocoeval.py:434-493)
    proposal_ar           the module-level _evaluate_predictions_ar (slender_det/evaluation/coco_evaluation.py:283-417)

Inputs are the flat forms the evaluator hands its kernels, so a test can feed the same predictions to both:
  gts   list of dicts with image_id, category_id (dataset id), bbox (XYWH), iscrowd, ratio, id, in json order;
  dets  dict of numpy arrays image_id, category_id (dataset id), bbox [N, 4] XYWH float32, score float32, in prediction order.
"""
import numpy as np
import torch

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
RATIO_RNG = [[0 / 1, 1e5 / 1], [0 / 1, 1 / 5], [1 / 5, 1 / 3], [1 / 3, 3 / 1], [3 / 1, 5 / 1], [5 / 1, 1e5 / 1]]
AR_RATIOS = [[0 / 1, 1e5 / 1], [0 / 1, 1 / 5], [1 / 5, 1 / 3], [1 / 3, 3 / 1], [3 / 1, 5 / 1], [5 / 1, 1e5 / 1]]
AR_AREAS = [[0, float("inf")], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, float("inf")]]


def _box_iou64(d, g, crowd):
    """[D, G] float64 overlaps of XYWH boxes; a crowd gt divides by the detection's area only."""
    out = np.zeros((len(d), len(g)))
    for j, (gx, gy, gw, gh) in enumerate(g):
        ga = gw * gh
        for i, (dx, dy, dw, dh) in enumerate(d):
            w = min(dx + dw, gx + gw) - max(dx, gx)
            if w <= 0:
                continue
            h = min(dy + dh, gy + gh) - max(dy, gy)
            if h <= 0:
                continue
            inter = w * h
            da = dw * dh
            out[i, j] = inter / (da if crowd[j] else da + ga - inter)
    return out


def _stable_desc(scores):
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind="mergesort")


def match_segment(gt_boxes, gt_crowd, gt_ratio, dt_boxes, dt_scores, max_det=100):
    """One (image, category): returns (order of the kept detections, matched [T, A, D] bool, ignored [T, A, D] bool,
    npig [A]).  Detections are taken in stable descending score order, at most max_det."""
    T, A = len(IOU_THRS), len(RATIO_RNG)
    order = _stable_desc(dt_scores)[:max_det]
    d = [tuple(float(v) for v in dt_boxes[i]) for i in order]
    g = [tuple(float(v) for v in b) for b in gt_boxes]
    G, D = len(g), len(d)
    ious = _box_iou64(d, g, gt_crowd) if (G and D) else None
    matched = np.zeros((T, A, D), bool)
    ignored = np.zeros((T, A, D), bool)
    npig = np.zeros(A, np.int64)
    for a, (lo, hi) in enumerate(RATIO_RNG):
        ig = np.array([bool(gt_crowd[j]) or gt_ratio[j] < lo or gt_ratio[j] > hi for j in range(G)], bool)
        npig[a] = int((~ig).sum())
        # gts with the ignore flag last, each half in its own order
        perm = [j for j in range(G) if not ig[j]] + [j for j in range(G) if ig[j]]
        for t, thr in enumerate(IOU_THRS):
            taken = np.zeros(G, bool)
            for i in range(D if ious is not None else 0):
                best, m = min(thr, 1 - 1e-10), -1
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
            r = d[i][2] / d[i][3]
            if r < lo or r > hi:
                ignored[:, a, i] |= ~matched[:, a, i]
    return order, matched, ignored, npig


def match_and_accumulate(img_ids, cat_ids, gts, dets):
    """precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M] (float64, -1 where a category has no gt
    in the range)."""
    img_ids, cat_ids = sorted(img_ids), sorted(cat_ids)
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(RATIO_RNG), len(MAX_DETS)
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
            dn = dseg.get((img, cat), [])
            if not g and not dn:
                continue
            sc = np.array([float(dets["score"][n]) for n in dn], np.float64)
            order, mt, ig, npig = match_segment([x["bbox"] for x in g], [int(x["iscrowd"]) for x in g], [x["ratio"] for x in g],
                                                dets["bbox"][dn] if dn else np.zeros((0, 4), np.float32), sc)
            per_img.append((sc[order], mt, ig, npig))
        if not per_img:
            continue
        for a in range(A):
            npig = int(sum(p[3][a] for p in per_img))
            if npig == 0:
                continue
            for m, md in enumerate(MAX_DETS):
                sc = np.concatenate([p[0][:md] for p in per_img])
                inds = _stable_desc(sc)
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


def summarize(precision, recall):
    """The 16 summary numbers: AP (all IoUs, all ratios, 100), AP50, AP75, AP per ratio range @100, AR @1/10/100, AR per
    ratio range @100; a mean over the entries > -1, or -1 when there are none."""
    def one(ap, t=None, a=0, m=2):
        s = precision if ap else recall
        if t is not None:
            s = s[np.where(t == IOU_THRS)[0]]
        s = s[:, :, :, [a], [m]] if ap else s[:, :, [a], [m]]
        v = s[s > -1]
        return -1 if len(v) == 0 else np.mean(v)

    out = [one(1), one(1, .5), one(1, .75)] + [one(1, a=a) for a in range(1, 6)]
    out += [one(0, m=0), one(0, m=1), one(0, m=2)] + [one(0, a=a) for a in range(1, 6)]
    return np.array(out)


def derive_bbox_results(stats, precision, class_names):
    res = {}
    for i, name in enumerate(["AP", "AP50", "AP75", "APs", "APm", "APl"]):
        res[name] = float(stats[i] * 100 if stats[i] >= 0 else "nan")
    if class_names is None or len(class_names) <= 1:
        return res
    res["AP-ratios"] = {"AP-" + n: precision[:, :, i, :, -1].mean(0).mean(0).tolist() for i, n in enumerate(class_names)}
    return res


def _xywh_to_xyxy32(b):
    t = torch.tensor([float(v) for v in b])
    t[2] += t[0]
    t[3] += t[1]
    return t


def _iou32(b1, b2):
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = (torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return torch.where(inter > 0, inter / (a1[:, None] + a2 - inter), torch.zeros(1))


def _in(v, lo, hi):
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    return bool(v >= lo32) and bool(v <= hi32)


def proposal_ar(images, gts_by_image, cat_to_contig, num_cats, limit=100):
    """images: list of (image_id, boxes XYWH float32 [D, 4], contiguous classes [D]) in prediction order.  Returns recalls
    [T, K+1, R, A] float32, ar, mar (0-dim float32), num_pos [K+1, R, A] int64.  Each image keeps its first `limit` boxes
    AND classes."""
    K, R, A = num_cats + 1, len(AR_RATIOS), len(AR_AREAS)
    thr = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)
    T = len(thr)
    hit = torch.zeros((T, K, R, A), dtype=torch.float32)
    cnt = torch.zeros((K, R, A), dtype=torch.float32)
    num_pos = torch.zeros((K, R, A), dtype=torch.int64)
    used = 0
    for image_id, boxes, classes in images:
        anno = [o for o in gts_by_image.get(image_id, []) if o["iscrowd"] == 0]
        if len(anno) == 0 or len(boxes) == 0:
            continue
        used += 1
        boxes, classes = boxes[:limit], classes[:limit]
        pb = torch.stack([_xywh_to_xyxy32(b) for b in boxes])
        gb = torch.stack([_xywh_to_xyxy32(o["bbox"]) for o in anno])
        gc = [cat_to_contig[o["category_id"]] for o in anno]
        gr = torch.tensor([o["ratio"] for o in anno], dtype=torch.float32)
        ga = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
        rs = [[r for r, (lo, hi) in enumerate(AR_RATIOS) if _in(gr[j], lo, hi)] for j in range(len(anno))]
        as_ = [[a for a, (lo, hi) in enumerate(AR_AREAS) if _in(ga[j], lo, hi)] for j in range(len(anno))]
        for j in range(len(anno)):
            for r in rs[j]:
                for a in as_[j]:
                    num_pos[gc[j], r, a] += 1
                    num_pos[K - 1, r, a] += 1
        ov = _iou32(pb, gb)
        same = torch.tensor([[int(c) == g for g in gc] for c in classes], dtype=torch.bool)
        ovm = ov * same
        img_hit = torch.zeros((T, K, R, A), dtype=torch.float32)
        for _ in range(min(len(boxes), len(anno))):
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
    return recalls, ar, mar, num_pos, used


def ar_results(recalls, ar, mar, num_pos, limit=100):
    """The "ar" result dict (coco_evaluation.py:238-280) with floats for values."""
    res = {}
    areas = ["all areas", "small", "medium", "large"]
    ratios = ["all ratios", " 0  - 1/5", "1/5 - 1/3", "1/3 - 3/1", "3/1 - 5/1", "5/1 - INF"]
    for i, key in enumerate(areas):
        res["AR-{}@{:d}".format(key, limit)] = float(recalls[:, -1, 0, i].mean() * 100)
        res["mAR-{}@{:d}".format(key, limit)] = float(recalls[:, :-1, 0, i].mean() * 100)
    for i, key in enumerate(ratios):
        res["AR-{}@{:d}".format(key, limit)] = float(recalls[:, -1, i, 0].mean() * 100)
        res["mAR-{}@{:d}".format(key, limit)] = float(recalls[:, :-1, i, 0].mean() * 100)
    res["AR@{:d}".format(limit)] = float(ar.item() * 100)
    res["mAR@{:d}".format(limit)] = float(mar.item() * 100)
    return res
