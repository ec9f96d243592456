"""The three HIP passes of the evaluation over flat device tensors (csrc/coco_eval.hip):

    match       sod_coco_match       COCOeval.computeIoU + evaluateImg, one wave per (category, image) segment
    accumulate  sod_coco_accumulate  COCOeval.accumulate, one workgroup per (category, ratio range, maxDets, IoU threshold)
    ar          sod_proposal_ar      _evaluate_predictions_ar, one workgroup per image

run_rotated is the rotated-box evaluation (detectron2's RotatedCOCOeval): sod_coco_match_rotated (csrc/coco_eval_rotated.hip) on
(cx, cy, w, h, angle) boxes with COCO's area ranges or the slenderness ranges, then the same sod_coco_accumulate.  run_rotated_ar is the
"ar" pass on those boxes (sod_proposal_ar_rotated): the rounds of sod_proposal_ar with the rotated IoU as the overlap.

Ordering uses stable device sorts on packed int64 keys (segment or category in the high word, -score mapped to an order-preserving
unsigned word in the low one): one sort puts every segment's detections in stable descending score order, a second gives each
category the stable -score order of its image-major concatenation that accumulate walks.
"""
import ctypes

import numpy as np
import torch

from .. import _C

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
RATIO_RNG = [[0 / 1, 1e5 / 1], [0 / 1, 1 / 5], [1 / 5, 1 / 3], [1 / 3, 3 / 1], [3 / 1, 5 / 1], [5 / 1, 1e5 / 1]]
RATIO_LBL = ["all", " 0  - 1/5", "1/5 - 1/3", "1/3 - 3", "3/1 - 5/1", "5/1 - INF"]
AR_RATIOS = {"all ratios": [0 / 1, 1e5 / 1], " 0  - 1/5": [0 / 1, 1 / 5], "1/5 - 1/3": [1 / 5, 1 / 3], "1/3 - 3/1": [1 / 3, 3 / 1],
             "3/1 - 5/1": [3 / 1, 5 / 1], "5/1 - INF": [5 / 1, 1e5 / 1]}
AR_AREAS = {"all areas": [0, float("inf")], "small": [0, 32 ** 2], "medium": [32 ** 2, 96 ** 2], "large": [96 ** 2, float("inf")]}
AR_LIMIT = 100
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]     # pycocotools Params.areaRng
AREA_LBL = ["all", "small", "medium", "large"]


def ar_thresholds():
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


def _hp(a):
    """Host pointer of a contiguous numpy array (parameters the C ABI reads on the host)."""
    return a.ctypes.data_as(ctypes.c_void_p)


def _desc_key(score):
    """int64 in [0, 2^32), ascending in -score (float32 order; -0.0 folded onto 0.0)."""
    b = (-score.float() + 0.0).view(torch.int32).to(torch.int64)
    return torch.where(b >= 0, b, b ^ 0x7FFFFFFF) + (1 << 31)


def _scratch_offsets(counts, per_item):
    """Per-item offsets into one scratch buffer for the items whose size (per_item(count), memoised per distinct count) is > 0."""
    sizes = np.zeros(len(counts), np.int64)
    for c in np.unique(counts):
        n = int(per_item(int(c)))
        if n < 0:
            raise _C.SlenderHipError("scratch size query failed")
        sizes[counts == c] = n
    off = np.zeros(len(counts), np.int64)
    if len(counts) > 1:
        np.cumsum(sizes[:-1], out=off[1:])
    return off, int(sizes.sum())


class GtDevice:
    """The gt arrays of a CocoGt on one device, with the scratch layout of both passes (built once per evaluator)."""

    def __init__(self, gt, device):
        lib = _C.load()
        h = gt.arrays()
        self.I, self.K = len(gt.img_ids), len(gt.cat_ids)
        if len(h["img_cls"]) and not (0 <= h["img_cls"].min() and h["img_cls"].max() < self.K):
            raise ValueError("thing_dataset_id_to_contiguous_id must map the categories onto 0 .. K-1")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        self._index(gt, t)
        self.seg_gt_off, self.seg_box, self.seg_crowd, self.seg_ratio = (t(h[k]) for k in ("seg_gt_off", "seg_box", "seg_crowd", "seg_ratio"))
        self.img_gt_off, self.img_box, self.img_cls, self.img_ratio = (t(h[k]) for k in ("img_gt_off", "img_box", "img_cls", "img_ratio"))
        off, n = _scratch_offsets(np.diff(h["seg_gt_off"]), lambda g: lib.sod_coco_match_scratch_doubles(g, MAX_DETS[-1]))
        self.match_scratch_off, self.match_scratch = t(off), torch.empty(max(n, 1), dtype=torch.float64, device=device)
        off, n = _scratch_offsets(np.diff(h["img_gt_off"]), lambda g: lib.sod_proposal_ar_scratch_floats(g, AR_LIMIT))
        self.ar_scratch_off, self.ar_scratch = t(off), torch.empty(max(n, 1), dtype=torch.float32, device=device)

    def _index(self, gt, t):
        self.img_ids = t(np.array(gt.img_ids, np.int64))
        # contiguous class id -> sorted category index k (-1: not a category of the dataset)
        cmax = max(gt.id_map.values()) if gt.id_map else 0
        c2k = np.full(cmax + 2, -1, np.int64)
        for cid, c in gt.id_map.items():
            if cid in gt.cat_ids:
                c2k[c] = gt.cat_ids.index(cid)
        self.contig_to_k = t(c2k)
        self.num_contig = max(gt.id_map.values()) + 1 if gt.id_map else 0


class RotatedGtDevice(GtDevice):
    """The gt arrays of CocoGt.rotated_arrays() on one device, with the scratch layout of the rotated match pass."""

    def __init__(self, gt, device):
        lib = _C.load()
        h = gt.rotated_arrays()
        self.I, self.K = len(gt.img_ids), len(gt.cat_ids)
        ids = [gt.id_map[c] for c in gt.cat_ids if c in gt.id_map]
        if ids and not (0 <= min(ids) and max(ids) < self.K):
            raise ValueError("thing_dataset_id_to_contiguous_id must map the categories onto 0 .. K-1")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        self._index(gt, t)
        self.seg_gt_off, self.seg_box5, self.seg_crowd, self.seg_area, self.seg_ratio5 = (
            t(h[k]) for k in ("seg_gt_off", "seg_box5", "seg_crowd", "seg_area", "seg_ratio5"))
        off, n = _scratch_offsets(np.diff(h["seg_gt_off"]), lambda g: lib.sod_coco_match_rotated_scratch_floats(g, MAX_DETS[-1]))
        self.match_scratch_off, self.match_scratch = t(off), torch.empty(max(n, 2), dtype=torch.float32, device=device)
        self._gt, self._device, self._recall = gt, device, None

    def recall(self):
        """The gt arrays of CocoGt.rotated_recall_arrays() on the device with the scratch layout of the rotated recall pass: built at the
        first call, so an evaluation without that pass neither uploads nor allocates them."""
        if self._recall is None:
            lib = _C.load()
            h = self._gt.rotated_recall_arrays()
            if len(h["img_cls"]) and not (0 <= h["img_cls"].min() and h["img_cls"].max() < self.K):
                raise ValueError("thing_dataset_id_to_contiguous_id must map the categories onto 0 .. K-1")
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self._device)  # noqa: E731
            r = {k: t(h[k]) for k in ("img_gt_off", "img_box5", "img_cls", "img_ratio5")}
            off, n = _scratch_offsets(np.diff(h["img_gt_off"]), lambda g: lib.sod_proposal_ar_rotated_scratch_floats(g, AR_LIMIT))
            r["scratch_off"], r["scratch"] = t(off), torch.empty(max(n, 1), dtype=torch.float32, device=self._device)
            self._recall = r
        return self._recall


def _ev(events, name):
    if events is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events.setdefault(name, []).append(e)


def _locate(gd, image_id, classes, check):
    """Image index ii, contiguous class cl and sorted category index k of every prediction (device tensors); with ``check`` a
    prediction that names an unknown image or category raises (one host synchronisation)."""
    I, K = gd.I, gd.K
    ii = torch.searchsorted(gd.img_ids, image_id) if I else torch.zeros_like(image_id)
    cl = classes.long()
    k = gd.contig_to_k[cl.clamp(0, gd.contig_to_k.numel() - 1)]
    if check:
        ok = (ii < I) & (gd.img_ids[ii.clamp(max=max(I - 1, 0))] == image_id) & (cl >= 0) & (cl < min(gd.num_contig, K)) & (k >= 0)
        if not bool(ok.all()):
            raise ValueError("a prediction names an image or a category that is not in the dataset")
    return ii, cl, k


def _segment_sort(gd, seg, scores):
    """perm1: the predictions by segment, stable descending score within; seg_s = seg[perm1]; dt_off [S+1]; rank in the segment."""
    dev = scores.device
    S, N = gd.K * gd.I, int(scores.shape[0])
    perm1 = torch.sort((seg << 32) | _desc_key(scores), stable=True).indices
    seg_s = seg[perm1]
    dt_off = torch.searchsorted(seg_s, torch.arange(S + 1, device=dev)).int()
    rank = (torch.arange(N, device=dev) - dt_off[seg_s.clamp(max=max(S - 1, 0))]).int()
    return perm1, seg_s, dt_off, rank


def _accumulate(gd, seg_s, score_s, rank, matched, ignored, npig, A, st):
    """sod_coco_accumulate over the segment-ordered match results: precision / scores [T, R, K, A, M], recall [T, K, A, M]."""
    dev = score_s.device
    I, K = gd.I, gd.K
    T, R, M = len(IOU_THRS), len(REC_THRS), len(MAX_DETS)
    k_s = seg_s // max(I, 1)
    perm2 = torch.sort((k_s << 32) | _desc_key(score_s), stable=True).indices
    cat_off = torch.searchsorted(k_s, torch.arange(K + 1, device=dev)).int()
    precision = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    recall = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    sc = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    md = np.array(MAX_DETS, np.int32)
    rt = np.ascontiguousarray(REC_THRS, np.float64)
    _C.call("sod_coco_accumulate", _C.ptr(cat_off), _C.ptr(perm2), _C.ptr(score_s), _C.ptr(rank), _C.ptr(matched), _C.ptr(ignored),
            _C.ptr(npig), K, T, A, _hp(md), M, _hp(rt), R, _C.ptr(precision), _C.ptr(recall), _C.ptr(sc), st)
    return precision, recall, sc


def _recall_pass(sym, gt, scratch_off, scratch, ii, cl, boxes, I, K, st):
    """The recall pass ``sym`` (sod_proposal_ar / sod_proposal_ar_rotated) over the predictions in prediction order: gt = (img_gt_off,
    boxes, classes, ratios) by image, ii / cl the image index and contiguous class of every prediction, boxes [N, 4 or 5] float32.
    Returns recalls [T, K+1, R, A] float32, counts [K+1, R, A] int32, hits [T, K+1, R, A] int32."""
    dev = boxes.device
    K1 = K + 1                                                     # the reference's len(cats) + 1, "all classes" last
    Ra, Aa = len(AR_RATIOS), len(AR_AREAS)
    perm3 = torch.sort(ii, stable=True).indices
    img_off = torch.searchsorted(ii[perm3], torch.arange(I + 1, device=dev)).int()
    thr = ar_thresholds().numpy()
    Ta = len(thr)
    rr = np.array(list(AR_RATIOS.values()), np.float32).reshape(-1)
    aa = np.array(list(AR_AREAS.values()), np.float32).reshape(-1)
    hits = torch.zeros((Ta, K1, Ra, Aa), dtype=torch.int32, device=dev)
    counts = torch.zeros((K1, Ra, Aa), dtype=torch.int32, device=dev)
    recalls = torch.empty((Ta, K1, Ra, Aa), dtype=torch.float32, device=dev)
    dt_cls = cl.int().contiguous()
    gt_off, gt_box, gt_cls, gt_ratio = gt
    _C.call(sym, _C.ptr(gt_off), _C.ptr(gt_box), _C.ptr(gt_cls), _C.ptr(gt_ratio), _C.ptr(img_off), _C.ptr(perm3), _C.ptr(boxes),
            _C.ptr(dt_cls), I, AR_LIMIT, K1, _hp(thr), Ta, _hp(rr), Ra, _hp(aa), Aa, _C.ptr(scratch_off), _C.ptr(scratch), _C.ptr(hits),
            _C.ptr(counts), _C.ptr(recalls), st)
    return recalls, counts, hits


def run(gd, image_id, boxes_xyxy, scores, classes, check=True, events=None):
    """image_id [N] int64, boxes_xyxy [N, 4] float32, scores [N] float32, classes [N] int64 contiguous ids - device tensors in
    prediction order.  Returns device tensors: precision / scores [T, R, K, A, M], recall [T, K, A, M] float64, recalls
    [T, K+1, R, A] float32, counts [K+1, R, A] int32, plus the intermediate match results."""
    dev = boxes_xyxy.device
    st = _C.stream_ptr()
    I, K, N = gd.I, gd.K, int(scores.shape[0])
    T, A = len(IOU_THRS), len(RATIO_RNG)
    b = boxes_xyxy.float()
    xywh = torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], dim=1).contiguous()      # instances_to_coco_json: XYXY -> XYWH in float32
    ii, cl, k = _locate(gd, image_id, classes, check and N)
    _ev(events, "match")
    S = K * I
    perm1, seg_s, dt_off, rank = _segment_sort(gd, k * I + ii, scores)
    box_s = xywh[perm1].contiguous()
    score_s = scores.float()[perm1].contiguous()
    matched = torch.zeros(N, dtype=torch.int64, device=dev)
    ignored = torch.zeros(N, dtype=torch.int64, device=dev)
    npig = torch.zeros(K * A, dtype=torch.int32, device=dev)
    iou_thr = np.ascontiguousarray(IOU_THRS, np.float64)
    rng = np.ascontiguousarray(np.array(RATIO_RNG, np.float64).reshape(-1))
    _C.call("sod_coco_match", _C.ptr(gd.seg_gt_off), _C.ptr(gd.seg_box), _C.ptr(gd.seg_crowd), _C.ptr(gd.seg_ratio), _C.ptr(dt_off),
            _C.ptr(box_s), S, max(I, 1), MAX_DETS[-1], _hp(iou_thr), T, _hp(rng), A, _C.ptr(gd.match_scratch_off),
            _C.ptr(gd.match_scratch), _C.ptr(matched), _C.ptr(ignored), _C.ptr(npig), st)
    _ev(events, "accumulate")
    precision, recall, sc = _accumulate(gd, seg_s, score_s, rank, matched, ignored, npig, A, st)
    _ev(events, "ar")
    recalls, counts, hits = _recall_pass("sod_proposal_ar", (gd.img_gt_off, gd.img_box, gd.img_cls, gd.img_ratio), gd.ar_scratch_off,
                                         gd.ar_scratch, ii, cl, xywh, I, K, st)
    _ev(events, "end")
    return {"precision": precision, "recall": recall, "scores": sc, "recalls": recalls, "counts": counts, "hits": hits,
            "dt_matched": matched, "dt_ignored": ignored, "npig": npig, "perm1": perm1, "rank": rank}


def run_rotated(gd, image_id, boxes5, scores, classes, bucket="area", check=True, events=None):
    """The rotated-box evaluation.  gd a RotatedGtDevice; image_id [N] int64, boxes5 [N, 5] float32 (cx, cy, w, h, angle_deg),
    scores [N] float32, classes [N] int64 contiguous ids - device tensors in prediction order.  ``bucket`` "area": COCO's four
    area ranges, a gt by its annotated area, a detection by w * h; "ratio": the six slenderness ranges, a gt by its side ratio,
    a detection by w / h.  Returns device tensors precision / scores [T, R, K, A, M], recall [T, K, A, M] float64 plus the
    intermediate match results."""
    if bucket not in ("area", "ratio"):
        raise ValueError(f"bucket must be 'area' or 'ratio', not {bucket!r}")
    dev = boxes5.device
    st = _C.stream_ptr()
    I, K, N = gd.I, gd.K, int(scores.shape[0])
    ranges = AREA_RNG if bucket == "area" else RATIO_RNG
    T, A = len(IOU_THRS), len(ranges)
    b = boxes5.float().reshape(-1, 5)
    w64, h64 = b[:, 2].double(), b[:, 3].double()
    val = w64 * h64 if bucket == "area" else w64 / h64             # pycocotools loadRes: area = bb[2] * bb[3]
    gt_val = gd.seg_area if bucket == "area" else gd.seg_ratio5
    ii, cl, k = _locate(gd, image_id, classes, check and N)
    _ev(events, "match")
    S = K * I
    perm1, seg_s, dt_off, rank = _segment_sort(gd, k * I + ii, scores)
    box_s = b[perm1].contiguous()
    val_s = val[perm1].contiguous()
    score_s = scores.float()[perm1].contiguous()
    matched = torch.zeros(N, dtype=torch.int64, device=dev)
    ignored = torch.zeros(N, dtype=torch.int64, device=dev)
    npig = torch.zeros(K * A, dtype=torch.int32, device=dev)
    iou_thr = np.ascontiguousarray(IOU_THRS, np.float64)
    rng = np.ascontiguousarray(np.array(ranges, np.float64).reshape(-1))
    _C.call("sod_coco_match_rotated", _C.ptr(gd.seg_gt_off), _C.ptr(gd.seg_box5), _C.ptr(gd.seg_crowd), _C.ptr(gt_val), _C.ptr(dt_off),
            _C.ptr(box_s), _C.ptr(val_s), S, max(I, 1), MAX_DETS[-1], _hp(iou_thr), T, _hp(rng), A, _C.ptr(gd.match_scratch_off),
            _C.ptr(gd.match_scratch), _C.ptr(matched), _C.ptr(ignored), _C.ptr(npig), st)
    _ev(events, "accumulate")
    precision, recall, sc = _accumulate(gd, seg_s, score_s, rank, matched, ignored, npig, A, st)
    _ev(events, "end")
    return {"precision": precision, "recall": recall, "scores": sc, "dt_matched": matched, "dt_ignored": ignored, "npig": npig,
            "perm1": perm1, "rank": rank, "dt_off": dt_off}


def run_rotated_ar(gd, image_id, boxes5, scores, classes, check=True, events=None):
    """The slenderness-bucketed recall pass (AR / mAR) on rotated boxes: sod_proposal_ar_rotated with the thresholds, the six ratio and
    four area ranges and the 100-detection limit of the axis-aligned pass.  gd a RotatedGtDevice; the arguments as run_rotated (the pass
    has no score order: ``scores`` only fixes the signature).  Returns device tensors recalls [T, K+1, R, A] float32, counts
    [K+1, R, A] int32, hits [T, K+1, R, A] int32."""
    st = _C.stream_ptr()
    N = int(scores.shape[0])
    b = boxes5.float().reshape(-1, 5).contiguous()
    r = gd.recall()
    ii, cl, _ = _locate(gd, image_id, classes, check and N)
    _ev(events, "ar")
    recalls, counts, hits = _recall_pass("sod_proposal_ar_rotated", (r["img_gt_off"], r["img_box5"], r["img_cls"], r["img_ratio5"]),
                                         r["scratch_off"], r["scratch"], ii, cl, b, gd.I, gd.K, st)
    _ev(events, "ar_end")
    return {"recalls": recalls, "counts": counts, "hits": hits}
