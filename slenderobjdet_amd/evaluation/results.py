"""Host-side summaries of the device arrays, with the reference's expressions (numpy float64 / torch CPU float32), so that the
numbers are the ones the reference prints:
    summarize             COCOeval.summarize's 16 stats (cocoeval.py:434-493)
    derive_coco_results   COCOEvaluator._derive_coco_results (coco_evaluation.py:166-236) for bbox
    ar_results            COCOEvaluator._evaluate_predictions_ar (coco_evaluation.py:238-280) + the module-level pass's tail (:391-417)
    summarize_area        pycocotools COCOeval.summarize's 12 stats over the area ranges (rotated-box evaluation)
    derive_rotated_results  detectron2 COCOEvaluator._derive_coco_results for bbox, as RotatedCOCOEvaluator reports it
    derive_ratio_results  the 16 stats of ``summarize`` as a dict (the rotated evaluator's slenderness extension)
"""
from collections import OrderedDict

import numpy as np
import torch

from .device import AR_AREAS, AR_LIMIT, AR_RATIOS, AREA_LBL, IOU_THRS, MAX_DETS, RATIO_LBL

BBOX_METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]


def summarize(precision, recall):
    def one(ap, iou_thr=None, rng="all", max_dets=100):
        aind = [i for i, lbl in enumerate(RATIO_LBL) if lbl == rng]
        mind = [i for i, m in enumerate(MAX_DETS) if m == max_dets]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    md = MAX_DETS
    stats = [one(1), one(1, iou_thr=.5, max_dets=md[2]), one(1, iou_thr=.75, max_dets=md[2])]
    stats += [one(1, rng=lbl, max_dets=md[2]) for lbl in RATIO_LBL[1:]]
    stats += [one(0, max_dets=md[0]), one(0, max_dets=md[1]), one(0, max_dets=md[2])]
    stats += [one(0, rng=lbl, max_dets=md[2]) for lbl in RATIO_LBL[1:]]
    return np.array(stats)


def derive_coco_results(stats, precision, class_names=None):
    """stats None: no predictions at all (every metric NaN).  stats[3:6] carry the reference's area labels APs / APm / APl
    although they are the 0-1/5, 1/5-1/3 and 1/3-3 ratio buckets; AP-ratios averages over T and R including the -1 entries."""
    if stats is None:
        return {m: float("nan") for m in BBOX_METRICS}
    results = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(BBOX_METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    assert len(class_names) == precision.shape[2]
    results["AP-ratios"] = {"AP-" + "{}".format(n): precision[:, :, i, :, -1].mean(0).mean(0).tolist() for i, n in enumerate(class_names)}
    return results


def summarize_area(precision, recall):
    """precision [T, R, K, 4, 3], recall [T, K, 4, 3] over the area ranges all / small / medium / large: AP, AP@.5, AP@.75,
    AP small / medium / large (100 detections), AR@1, AR@10, AR@100, AR small / medium / large (100)."""
    def one(ap, iou_thr=None, rng="all", max_dets=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == rng]
        mind = [i for i, m in enumerate(MAX_DETS) if m == max_dets]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    md = MAX_DETS
    stats = [one(1), one(1, iou_thr=.5, max_dets=md[2]), one(1, iou_thr=.75, max_dets=md[2])]
    stats += [one(1, rng=lbl, max_dets=md[2]) for lbl in AREA_LBL[1:]]
    stats += [one(0, max_dets=md[0]), one(0, max_dets=md[1]), one(0, max_dets=md[2])]
    stats += [one(0, rng=lbl, max_dets=md[2]) for lbl in AREA_LBL[1:]]
    return np.array(stats)


def derive_rotated_results(stats, precision, class_names=None):
    """stats None: no predictions at all (every metric NaN).  With more than one class name also "AP-<name>": the mean of the
    class's precision over all IoU thresholds and recall thresholds at area "all", 100 detections (NaN without any entry > -1)."""
    if stats is None:
        return {m: float("nan") for m in BBOX_METRICS}
    results = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(BBOX_METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    assert len(class_names) == precision.shape[2]
    for i, n in enumerate(class_names):
        p = precision[:, :, i, 0, -1]
        p = p[p > -1]
        results["AP-" + "{}".format(n)] = float(np.mean(p) * 100) if p.size else float("nan")
    return results


def ratio_result_keys():
    return (["AP", "AP50", "AP75"] + ["AP-" + lbl for lbl in RATIO_LBL[1:]] + ["AR@{:d}".format(m) for m in MAX_DETS]
            + ["AR-" + lbl for lbl in RATIO_LBL[1:]])


def derive_ratio_results(stats):
    """The 16 stats of ``summarize`` by name, x 100, NaN for -1 (stats None: every metric NaN)."""
    keys = ratio_result_keys()
    if stats is None:
        return {k: float("nan") for k in keys}
    return {k: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, k in enumerate(keys)}


def ar_results(recalls, num_pos, limit=AR_LIMIT):
    """recalls [T, K+1, R, A] float32 (CPU), num_pos [K+1, R, A] int64."""
    ar = recalls[:, -1, 0, 0].mean()
    mar = recalls[:, :-1, 0, 0].mean()
    res = OrderedDict()
    for i, key in enumerate(AR_AREAS):
        res["AR-{}@{:d}".format(key, limit)] = float(recalls[:, -1, 0, i].mean() * 100)
        res["mAR-{}@{:d}".format(key, limit)] = float(recalls[:, :-1, 0, i].mean() * 100)
    for i, key in enumerate(AR_RATIOS):
        res["AR-{}@{:d}".format(key, limit)] = float(recalls[:, -1, i, 0].mean() * 100)
        res["mAR-{}@{:d}".format(key, limit)] = float(recalls[:, :-1, i, 0].mean() * 100)
    res["AR@{:d}".format(limit)] = float(ar.item() * 100)
    res["mAR@{:d}".format(limit)] = float(mar.item() * 100)
    from .device import ar_thresholds

    res["ar-stats"] = {"ar": ar, "mar": mar, "thresholds": ar_thresholds(), "gt_overlaps": [], "num_pos": num_pos}
    return res


def as_cpu_recalls(recalls):
    return torch.as_tensor(recalls).detach().to("cpu", torch.float32).contiguous()
