"""Test-time augmentation restated in numpy float64 (detectron2's source is absent; DESIGN.md section 12 states the semantics):
the DatasetMapperTTA plan, the un-flip / scale / clip / threshold of the augmented detections, and the merging NMS (class-aware greedy
suppression of IoU > threshold in stable descending-score order, then top-k).  Independent of the product code: only numpy."""
import numpy as np


def plan(h, w, min_sizes, max_size, flip):
    """[(newh, neww, flip)] : per min size the resized run, then the resized + mirrored one (ResizeShortestEdge.get_transform sizes)."""
    out = []
    for size in min_sizes:
        scale = size * 1.0 / min(h, w)
        newh, neww = (size, scale * w) if h < w else (scale * h, size)
        if max(newh, neww) > max_size:
            s = max_size * 1.0 / max(newh, neww)
            newh, neww = newh * s, neww * s
        newh, neww = int(newh + 0.5), int(neww + 0.5)
        out.append((newh, neww, False))
        if flip:
            out.append((newh, neww, True))
    return out


def unmap(boxes, scores, classes, aug_hw, flip, out_hw, score_thresh):
    """One run's detections in the augmented image (h_a, w_a) -> the candidates at out_hw = (H, W).  Returns (boxes float64 (n, 4),
    scores, classes, valid bool (n)); rows with valid = False are the ones the merge drops (non-finite, score <= score_thresh)."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4).copy()
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    c = np.asarray(classes).reshape(-1).astype(np.int64)
    (ha, wa), (H, W) = aug_hw, out_hw
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(b).all(axis=1) & np.isfinite(s) & (s > score_thresh)
    b[~valid] = 0.0
    if flip:
        x1 = wa - b[:, 2]
        x2 = wa - b[:, 0]
        b[:, 0], b[:, 2] = x1, x2
    b[:, 0::2] *= W / wa
    b[:, 1::2] *= H / ha
    b[:, 0::2] = np.clip(b[:, 0::2], 0.0, W)
    b[:, 1::2] = np.clip(b[:, 1::2], 0.0, H)
    return b, s, c, valid


def merge_candidates(runs, out_hw, score_thresh):
    """runs: [(boxes, scores, classes, (h_a, w_a), flip)] in augmentation order -> concatenated valid candidates (boxes, scores, classes,
    run index of every candidate), order preserved."""
    B, S, C, R = [np.zeros((0, 4))], [np.zeros(0)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for r, (boxes, scores, classes, aug_hw, flip) in enumerate(runs):
        b, s, c, v = unmap(boxes, scores, classes, aug_hw, flip, out_hw, score_thresh)
        B.append(b[v]); S.append(s[v]); C.append(c[v]); R.append(np.full(int(v.sum()), r, dtype=np.int64))
    return np.concatenate(B), np.concatenate(S), np.concatenate(C), np.concatenate(R)


def iou(a, b):
    """IoU of two XYXY boxes (float64); 0 for an empty intersection."""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def nms_topk(boxes, scores, classes, thresh, max_keep):
    """Kept indices: stable descending-score order, a box is suppressed by a kept box of its class with IoU > thresh; first max_keep."""
    order = np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")
    keep = []
    for i in order:
        if all(classes[i] != classes[j] or iou(boxes[i], boxes[j]) <= thresh for j in keep):
            keep.append(int(i))
    return keep[:max_keep]


def same_class_iou_margin(boxes, classes, thresh):
    """min |IoU - thresh| over ALL same-class pairs (inf without a pair)."""
    m = np.inf
    for i in range(len(boxes)):
        for j in range(i + 1, len(boxes)):
            if classes[i] == classes[j]:
                m = min(m, abs(iou(boxes[i], boxes[j]) - thresh))
    return m


def tta(runs, out_hw, score_thresh, nms_thresh, max_keep):
    """The whole merge: -> (boxes, scores, classes) of the final detections, score-descending."""
    b, s, c, _ = merge_candidates(runs, out_hw, score_thresh)
    keep = nms_topk(b, s, c, nms_thresh, max_keep)
    return b[keep], s[keep], c[keep]
