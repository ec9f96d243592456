"""RotatedCOCOEvaluator of detectron2 (rotated_coco_evaluation.py: RotatedCOCOeval.computeIoU under pycocotools' COCOeval), the
evaluator the reference's train_net.py:60-62 builds for datasets of evaluator type "rotated_coco" - on device.

Boxes are (cx, cy, w, h, angle_deg).  The IoU is pairwise_iou_rotated(detections, gts) in float32, the ranges are COCO's area
ranges (all / small / medium / large), the summary is pycocotools' 12 numbers, and the result is ``{"bbox": {AP, AP50, AP75, APs,
APm, APl[, AP-<class>]}}``.  process() is the base class's: nothing leaves the device before evaluate().

Kept from detectron2 / pycocotools: the parameters, the stable score order with the first 100 detections of an (image, category),
the greedy scan with ties to the later gt and ignored gts last, a dataset with rotated gts and crowd gts refused.  Deviations: a gt
without ``area`` takes w * h (pycocotools raises); a prediction tensor with four columns is read as XYXY.

``ratio_buckets=True`` is an extension, not reference behaviour: the match pass runs a second time with the six slenderness
ranges of the axis-aligned evaluator (a gt by ``ratio`` or min(w, h) / max(w, h) of its box, a detection by w / h) and
``results["bbox-ratios"]`` holds the 16 ratio-bucketed AP / AR numbers.

``MetadataCatalog.get(name).rotated_recall = True`` adds the slenderness-bucketed recall pass of the axis-aligned evaluator on
rotated boxes (sod_proposal_ar_rotated): ``results["ar"]`` with the keys of COCOEvaluator's - AR / mAR per area range and per ratio
range at 100 detections - follows the keys above and ``self.recalls`` holds the [T, K+1, R, A] recalls.  A gt's area bucket is
decided by w * h of its box, its ratio bucket by ``ratio`` or min(w, h) / max(w, h).  The switch travels in the metadata, as
``ratio_device`` does: the constructor keeps its parameters.
"""
import json
import os
from collections import OrderedDict

import torch

from . import device as D
from .coco_evaluation import COCOEvaluator
from .results import ar_results, derive_ratio_results, derive_rotated_results, summarize, summarize_area


def boxes_to_rotated(boxes):
    """[n, 5] float32 (cx, cy, w, h, angle_deg) from [n, 5] boxes as they are or [n, 4] XYXY boxes (XYXY -> XYWH -> centre form,
    each step in float32, angle 0)."""
    b = boxes.float()
    if b.shape[-1] == 5:
        return b.reshape(-1, 5)
    if b.shape[-1] != 4:
        raise ValueError(f"boxes must have 4 (XYXY) or 5 (cx, cy, w, h, angle) columns, not {tuple(boxes.shape)}")
    b = b.reshape(-1, 4)
    wh = b[:, 2:] - b[:, :2]
    return torch.cat([b[:, :2] + wh / 2, wh, torch.zeros_like(wh[:, :1])], dim=1)


class RotatedCOCOEvaluator(COCOEvaluator):
    def __init__(self, dataset_name, cfg=None, distributed=True, output_dir=None, ratio_buckets=False):
        """As COCOEvaluator; the json's ``bbox`` entries hold five numbers (cx, cy, w, h, angle_deg) or four (XYWH, angle 0).
        Raises ValueError for a dataset with both rotated boxes and crowd annotations."""
        super().__init__(dataset_name, cfg, distributed, output_dir)
        self._ratio_buckets = bool(ratio_buckets)
        self._gt.rotated_arrays()
        self.ratio_stats = self.ratio_precision = self.ratio_recall = None
        self._rotated_recall = bool(self._metadata.get("rotated_recall", False))
        self.recalls = None

    def _flat(self):
        if not self._chunks:
            return None
        dev = self._chunks[0][1].device
        cat = lambda i, dt: torch.cat([c[i].to(dev, dt) for c in self._chunks])  # noqa: E731
        return {"image_id": cat(0, torch.int64), "boxes": torch.cat([boxes_to_rotated(c[1].to(dev)) for c in self._chunks]),
                "scores": cat(2, torch.float32), "classes": cat(3, torch.int64)}

    def evaluate_flat(self, flat, events=None):
        """The match and accumulate passes over flat device arrays (image_id, boxes [N, 5] or XYXY [N, 4], scores, classes
        contiguous) in prediction order."""
        boxes = boxes_to_rotated(flat["boxes"])
        dev = boxes.device
        results = OrderedDict()
        if not self._do_evaluation:
            return results
        if self._gt_dev is None or self._gt_dev.img_ids.device != dev:
            self._gt_dev = D.RotatedGtDevice(self._gt, dev)
        out = D.run_rotated(self._gt_dev, flat["image_id"], boxes, flat["scores"], flat["classes"], bucket="area", events=events)
        self.precision = out["precision"].cpu().numpy()
        self.recall = out["recall"].cpu().numpy()
        self.scores = out["scores"].cpu().numpy()
        empty = flat["scores"].shape[0] == 0
        self.stats = None if empty else summarize_area(self.precision, self.recall)
        results["bbox"] = derive_rotated_results(self.stats, self.precision, self._gt.class_names)
        if self._ratio_buckets:
            out = D.run_rotated(self._gt_dev, flat["image_id"], boxes, flat["scores"], flat["classes"], bucket="ratio", check=False)
            self.ratio_precision = out["precision"].cpu().numpy()
            self.ratio_recall = out["recall"].cpu().numpy()
            self.ratio_stats = None if empty else summarize(self.ratio_precision, self.ratio_recall)
            results["bbox-ratios"] = derive_ratio_results(self.ratio_stats)
        if self._rotated_recall:
            out = D.run_rotated_ar(self._gt_dev, flat["image_id"], boxes, flat["scores"], flat["classes"], check=False, events=events)
            self.recalls = out["recalls"].cpu()
            results["ar"] = ar_results(self.recalls, out["counts"].cpu().to(torch.int64))
        return results

    def _write_results_json(self, flat):
        rev = {v: k for k, v in self._gt.id_map.items()}
        box5 = boxes_to_rotated(flat["boxes"]).cpu().tolist()
        res = [{"image_id": i, "category_id": rev[c], "bbox": bb, "score": s}
               for i, c, bb, s in zip(flat["image_id"].cpu().tolist(), flat["classes"].cpu().tolist(), box5, flat["scores"].cpu().tolist())]
        with open(os.path.join(self._output_dir, "coco_instances_results.json"), "w") as f:
            f.write(json.dumps(res))


__all__ = ["RotatedCOCOEvaluator", "boxes_to_rotated"]
