"""COCOEvaluator of slender_det/evaluation/coco_evaluation.py:29-281 for bbox: COCO AP / AR bucketed by the gt aspect ratio
instead of the area, and the greedy recall pass bucketed by ratio and area - on device (evaluation/device.py).

process() keeps each image's boxes, scores, classes and image id on the device without any host synchronisation; evaluate()
concatenates once, runs the three HIP passes and summarises on the host.
"""
import json
import logging
import os
from collections import OrderedDict

import torch

from ..data.catalog import MetadataCatalog
from ..utils import comm
from . import device as D
from .coco_gt import CocoGt
from .evaluator import DatasetEvaluator
from .results import ar_results, derive_coco_results, summarize


def _tasks_from_config(cfg):
    tasks = ("bbox",)
    model = getattr(cfg, "MODEL", None) if cfg is not None else None
    if model is not None and getattr(model, "MASK_ON", False):
        tasks = tasks + ("segm",)
    if model is not None and getattr(model, "KEYPOINT_ON", False):
        tasks = tasks + ("keypoints",)
    return tasks


class COCOEvaluator(DatasetEvaluator):
    def __init__(self, dataset_name, cfg=None, distributed=True, output_dir=None):
        """dataset_name's metadata must carry ``json_file`` (a COCO-format json); ``thing_dataset_id_to_contiguous_id`` and
        ``thing_classes`` are used when present (else the identity map over the sorted category ids).  Only bbox is evaluated:
        a config that asks for segm or keypoints raises NotImplementedError.  A ``ratio_device`` entry of the metadata ("cuda", "cpu")
        is handed to CocoGt: the gt ratios then come from structures.polygons.oriented_ratios, one kernel launch on a GPU, instead
        of the host loop (the constructor keeps the reference's four parameters, so the option travels beside json_file)."""
        self._tasks = _tasks_from_config(cfg)
        extra = [t for t in self._tasks if t != "bbox"]
        if extra:
            raise NotImplementedError(f"COCOEvaluator evaluates bbox only, not {extra}")
        self._distributed = distributed
        self._output_dir = output_dir
        self._logger = logging.getLogger(__name__)
        self._metadata = MetadataCatalog.get(dataset_name)
        if "json_file" not in self._metadata:
            raise ValueError(f"MetadataCatalog entry '{dataset_name}' has no json_file (a COCO-format annotation file)")
        self._gt = CocoGt(self._metadata["json_file"], id_map=self._metadata.get("thing_dataset_id_to_contiguous_id"),
                          class_names=self._metadata.get("thing_classes"), ratio_device=self._metadata.get("ratio_device"))
        self._do_evaluation = self._gt.has_annotations
        self._gt_dev = None
        self.stats = None
        self.precision = self.recall = self.scores = None
        self.reset()

    def reset(self):
        self._chunks = []       # per processed image: (image_id [n], boxes [n, 4], scores [n], classes [n]) on the device
        self._num_images = 0

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            self._num_images += 1
            if "instances" not in out:
                continue
            inst = out["instances"]
            boxes = inst.pred_boxes.tensor
            n = boxes.shape[0]
            img = torch.full((n,), int(inp["image_id"]), dtype=torch.int64, device=boxes.device)
            self._chunks.append((img, boxes, inst.scores, inst.pred_classes))

    def _flat(self):
        if not self._chunks:
            return None
        dev = self._chunks[0][1].device
        cat = lambda i, dt: torch.cat([c[i].to(dev, dt) for c in self._chunks])  # noqa: E731
        return {"image_id": cat(0, torch.int64), "boxes": cat(1, torch.float32).reshape(-1, 4), "scores": cat(2, torch.float32),
                "classes": cat(3, torch.int64)}

    def _gather(self):
        """(number of processed images, flat prediction arrays or None) on the main process; (0, None) elsewhere."""
        flat = self._flat()
        if not (self._distributed and comm.get_world_size() > 1):
            return self._num_images, flat
        comm.synchronize()
        cpu = None if flat is None else {k: v.cpu() for k, v in flat.items()}
        parts = comm.gather((self._num_images, cpu), dst=0)
        if not comm.is_main_process():
            return 0, None
        n = sum(p[0] for p in parts)
        got = [p[1] for p in parts if p[1] is not None]
        if not got:
            return n, None
        dev = flat["boxes"].device if flat is not None else (torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        return n, {k: torch.cat([g[k] for g in got]).to(dev) for k in got[0]}

    def evaluate(self, name="coco"):
        n_images, flat = self._gather()
        if self._distributed and comm.get_world_size() > 1 and not comm.is_main_process():
            return {}
        if n_images == 0:
            self._logger.warning("[COCOEvaluator] Did not receive valid predictions.")
            return {}
        if flat is None:
            dev = torch.device("cuda")
            flat = {"image_id": torch.zeros(0, dtype=torch.int64, device=dev), "boxes": torch.zeros((0, 4), device=dev),
                    "scores": torch.zeros(0, device=dev), "classes": torch.zeros(0, dtype=torch.int64, device=dev)}
        if self._output_dir:
            os.makedirs(os.path.join(self._output_dir, name), exist_ok=True)
            torch.save({k: v.cpu() for k, v in flat.items()}, os.path.join(self._output_dir, name, "instances_predictions.pth"))
            self._write_results_json(flat)
        return self.evaluate_flat(flat)

    def evaluate_flat(self, flat, events=None):
        """The three passes over flat device arrays (image_id, boxes XYXY, scores, classes contiguous) in prediction order."""
        dev = flat["boxes"].device
        if self._gt_dev is None or self._gt_dev.img_ids.device != dev:
            self._gt_dev = D.GtDevice(self._gt, dev)
        out = D.run(self._gt_dev, flat["image_id"], flat["boxes"], flat["scores"], flat["classes"], events=events)
        results = OrderedDict()
        recalls = out["recalls"].cpu()
        results["ar"] = ar_results(recalls, out["counts"].cpu().to(torch.int64))
        self.recalls = recalls
        if not self._do_evaluation:
            return results
        self.precision = out["precision"].cpu().numpy()
        self.recall = out["recall"].cpu().numpy()
        self.scores = out["scores"].cpu().numpy()
        if flat["scores"].shape[0] == 0:
            self.stats = None
            results["bbox"] = derive_coco_results(None, None)
        else:
            self.stats = summarize(self.precision, self.recall)
            results["bbox"] = derive_coco_results(self.stats, self.precision, self._gt.class_names)
        return results

    def _write_results_json(self, flat):
        rev = {v: k for k, v in self._gt.id_map.items()}
        b = flat["boxes"].float()
        xywh = torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], dim=1).cpu().tolist()
        res = [{"image_id": i, "category_id": rev[c], "bbox": bb, "score": s}
               for i, c, bb, s in zip(flat["image_id"].cpu().tolist(), flat["classes"].cpu().tolist(), xywh, flat["scores"].cpu().tolist())]
        with open(os.path.join(self._output_dir, "coco_instances_results.json"), "w") as f:
            f.write(json.dumps(res))


def predictions_from_numpy(preds, device):
    """Flat device arrays from the numpy dict of evaluation.synthetic (tests, tools)."""
    return {"image_id": torch.from_numpy(preds["image_id"]).to(device), "boxes": torch.from_numpy(preds["boxes"]).to(device),
            "scores": torch.from_numpy(preds["score"]).to(device), "classes": torch.from_numpy(preds["category"]).to(device)}


__all__ = ["COCOEvaluator", "predictions_from_numpy"]
