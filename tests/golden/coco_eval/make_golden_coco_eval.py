#!/usr/bin/env python
"""Generates the golden vectors of the slender-object COCO evaluation under tests/golden/coco_eval/ by running the
REFERENCE's own Python (read-only, from /root/reference) on synthetic cases.  Runs only where /root/reference exists; nothing
from the reference is copied: only inputs / outputs (numpy arrays, json strings) are written.

Recipe of tests/golden/make_golden.py: the reference files are loaded with importlib under stub modules
written here -
    slender_det/evaluation/cocoeval.py           whole file (COCOeval.evaluate / accumulate / summarize)
    slender_det/evaluation/coco.py               COCO.createIndex / compute_ratio
    slender_det/evaluation/coco_evaluation.py    _evaluate_predictions_ar, COCOEvaluator._derive_coco_results /
                                                 COCOEvaluator._evaluate_predictions_ar
- and the third-party pieces they call are restated from their documented behaviour:
    pycocotools COCO (dict constructor, getAnnIds / getImgIds / getCatIds / loadAnns, loadRes for bbox results),
    pycocotools.mask.iou for XYWH boxes (float64), detectron2 BoxMode.convert / Boxes / pairwise_iou (float32),
    concern.support.between / between_ranges (the real module needs cv2).

    python tests/golden/coco_eval/make_golden_coco_eval.py      # rewrites tests/golden/coco_eval/*.npz + meta.json
"""
import copy
import importlib.util
import itertools
import json
import os
import sys
import types
from collections import defaultdict

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(OUT)))
sys.path.insert(0, ROOT)

from slenderobjdet_amd.evaluation.synthetic import preds_xywh, synthetic_coco  # noqa: E402

RESTATED = "pycocotools COCO / loadRes, pycocotools.mask.iou (bbox), detectron2 BoxMode.convert / Boxes / pairwise_iou, concern.support.between(_ranges)"


def _stub(name, **attrs):
    m = sys.modules.get(name) or types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    m.__path__ = []
    sys.modules[name] = m
    return m


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# ---- pycocotools.coco.COCO, restated ----
class CocoApi:
    def __init__(self, annotation_file=None):
        self.dataset, self.anns, self.cats, self.imgs = {}, {}, {}, {}
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        if annotation_file is not None:
            self.dataset = annotation_file if isinstance(annotation_file, dict) else json.load(open(annotation_file))
            self.createIndex()

    def createIndex(self):
        anns, cats, imgs = {}, {}, {}
        imgToAnns, catToImgs = defaultdict(list), defaultdict(list)
        for ann in self.dataset.get("annotations", []):
            imgToAnns[ann["image_id"]].append(ann)
            anns[ann["id"]] = ann
        for img in self.dataset.get("images", []):
            imgs[img["id"]] = img
        for cat in self.dataset.get("categories", []):
            cats[cat["id"]] = cat
        if "annotations" in self.dataset and "categories" in self.dataset:
            for ann in self.dataset["annotations"]:
                catToImgs[ann["category_id"]].append(ann["image_id"])
        self.anns, self.imgToAnns, self.catToImgs, self.imgs, self.cats = anns, imgToAnns, catToImgs, imgs, cats

    def getAnnIds(self, imgIds=[], catIds=[], areaRng=[], iscrowd=None):
        imgIds = imgIds if isinstance(imgIds, (list, tuple, np.ndarray)) else [imgIds]
        catIds = catIds if isinstance(catIds, (list, tuple, np.ndarray)) else [catIds]
        if len(imgIds) == len(catIds) == len(areaRng) == 0:
            anns = self.dataset["annotations"]
        else:
            if len(imgIds):
                anns = list(itertools.chain.from_iterable(self.imgToAnns[i] for i in imgIds if i in self.imgToAnns))
            else:
                anns = self.dataset["annotations"]
            anns = anns if len(catIds) == 0 else [a for a in anns if a["category_id"] in catIds]
            anns = anns if len(areaRng) == 0 else [a for a in anns if areaRng[0] < a["area"] < areaRng[1]]
        if iscrowd is not None:
            return [a["id"] for a in anns if a["iscrowd"] == iscrowd]
        return [a["id"] for a in anns]

    def getCatIds(self, catNms=[], supNms=[], catIds=[]):
        return [c["id"] for c in self.dataset["categories"]]

    def getImgIds(self, imgIds=[], catIds=[]):
        return list(self.imgs.keys())

    def loadAnns(self, ids=[]):
        return [self.anns[i] for i in ids] if isinstance(ids, (list, tuple, np.ndarray)) else [self.anns[ids]]

    def loadRes(self, resFile):
        res = CocoApi()
        res.dataset["images"] = [img for img in self.dataset["images"]]
        anns = resFile
        ids = [a["image_id"] for a in anns]
        assert set(ids) == (set(ids) & set(self.getImgIds())), "Results do not correspond to current coco set"
        res.dataset["categories"] = copy.deepcopy(self.dataset["categories"])
        for i, ann in enumerate(anns):
            bb = ann["bbox"]
            x1, x2, y1, y2 = [bb[0], bb[0] + bb[2], bb[1], bb[1] + bb[3]]
            if "segmentation" not in ann:
                ann["segmentation"] = [[x1, y1, x1, y2, x2, y2, x2, y1]]
            ann["area"] = bb[2] * bb[3]
            ann["id"] = i + 1
            ann["iscrowd"] = 0
        res.dataset["annotations"] = anns
        res.createIndex()
        return res


def mask_iou(d, g, iscrowd):
    """pycocotools.mask.iou on XYWH boxes (bbIou): float64, a crowd gt divides by the detection's area."""
    if len(d) == 0 or len(g) == 0:
        return []
    o = np.zeros((len(d), len(g)))
    for j, G in enumerate(g):
        ga = G[2] * G[3]
        for i, D in enumerate(d):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i_ = w * h
            u = da if iscrowd[j] else da + ga - i_
            o[i, j] = i_ / u
    return o


# ---- detectron2 structures, restated ----
class BoxMode:
    XYXY_ABS, XYWH_ABS = 0, 1

    @staticmethod
    def convert(box, from_mode, to_mode):
        assert isinstance(box, (list, tuple)) and len(box) == 4
        arr = torch.tensor(box)[None, :]
        if from_mode == BoxMode.XYWH_ABS and to_mode == BoxMode.XYXY_ABS:
            arr[:, 2] += arr[:, 0]
            arr[:, 3] += arr[:, 1]
        elif from_mode == BoxMode.XYXY_ABS and to_mode == BoxMode.XYWH_ABS:
            arr[:, 2] -= arr[:, 0]
            arr[:, 3] -= arr[:, 1]
        else:
            assert from_mode == to_mode
        return type(box)(arr.flatten().tolist())


class Boxes:
    def __init__(self, tensor):
        self.tensor = torch.as_tensor(tensor, dtype=torch.float32).reshape(-1, 4)

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, item):
        return Boxes(self.tensor[item])

    def __iter__(self):
        yield from self.tensor

    def area(self):
        b = self.tensor
        return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def pairwise_iou(boxes1, boxes2):
    area1, area2 = boxes1.area(), boxes2.area()
    b1, b2 = boxes1.tensor, boxes2.tensor
    wh = torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])
    wh.clamp_(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


# ---- concern.support, restated ----
def between(a, a_range):
    if isinstance(a, np.ndarray):
        return np.logical_and(a >= a_range[0], a <= a_range[1])
    return a >= a_range[0] and a <= a_range[1]


def between_ranges(a, ranges):
    return [between(a, r) for r in ranges]


class _Meta(dict):
    def __getattr__(self, k):
        if k in self:
            return self[k]
        raise AttributeError(k)


def install():
    np.float = float   # removed in numpy >= 1.24; accumulate() still spells it
    _stub("pycocotools")
    _stub("pycocotools.coco", COCO=CocoApi)
    _stub("pycocotools.mask", iou=mask_iou)
    sys.modules["pycocotools"].mask = sys.modules["pycocotools.mask"]
    _stub("detectron2")
    _stub("detectron2.structures", RotatedBoxes=None, BoxMode=BoxMode, Boxes=Boxes, pairwise_iou=pairwise_iou)
    _stub("detectron2.utils")
    _stub("detectron2.utils.comm", synchronize=lambda: None, gather=lambda x, dst=0: [x], is_main_process=lambda: True)
    _stub("detectron2.utils.logger", create_small_table=lambda d: "")
    _stub("detectron2.data", MetadataCatalog=None)
    _stub("detectron2.data.datasets")
    _stub("detectron2.data.datasets.coco", convert_to_coco_json=None)
    _stub("detectron2.evaluation", COCOEvaluator=object)
    _stub("fvcore")
    _stub("fvcore.common")
    _stub("fvcore.common.file_io", PathManager=None)
    _stub("slender_det")
    _stub("slender_det.structures")
    _stub("slender_det.structures.masks", PolygonMasks=None)
    _stub("concern")
    _stub("concern.support", between=between, between_ranges=between_ranges, rbox_from_polygon=None)
    _stub("refeval")
    ce = _load("refeval.cocoeval", "slender_det/evaluation/cocoeval.py")
    co = _load("refeval.coco", "slender_det/evaluation/coco.py")
    ev = _load("refeval.coco_evaluation", "slender_det/evaluation/coco_evaluation.py")
    return ce, co, ev


# ---- cases ----
AR_RATIOS = {"all ratios": [0 / 1, 1e5 / 1], " 0  - 1/5": [0 / 1, 1 / 5], "1/5 - 1/3": [1 / 5, 1 / 3], "1/3 - 3/1": [1 / 3, 3 / 1],
             "3/1 - 5/1": [3 / 1, 5 / 1], "5/1 - INF": [5 / 1, 1e5 / 1]}      # the argument COCOEvaluator._evaluate_predictions_ar passes
AR_AREAS = {"all areas": [0, float("inf")], "small": [0, 32 ** 2], "medium": [32 ** 2, 96 ** 2], "large": [96 ** 2, float("inf")]}


def _case_general():
    ds, pr = synthetic_coco(11, n_images=40, n_cats=6, dets_per_image=(0, 30))
    cats = sorted(c["id"] for c in ds["categories"])
    ds["annotations"] = [a for a in ds["annotations"] if a["category_id"] != cats[2]]     # a category with no gt
    return ds, pr


def _case_ties():
    return synthetic_coco(12, n_images=30, n_cats=4, dets_per_image=(0, 25), score_levels=5, dup=0.25)


def _case_boundaries():
    ds, pr = synthetic_coco(13, n_images=12, n_cats=3, dets_per_image=(5, 20), no_gt=0.0, no_dt=0.0)
    cats = sorted(c["id"] for c in ds["categories"])
    img = ds["images"][0]["id"]
    nid = max(a["id"] for a in ds["annotations"]) + 1
    extra = [  # (x, y, w, h, explicit ratio or None)
        (10, 10, 10, 50, None), (40, 10, 50, 10, None), (100, 10, 10, 30, None), (130, 10, 30, 10, None),
        (170, 10, 40, 40, None), (10, 100, 32, 32, None), (60, 100, 16, 64, None), (100, 100, 96, 96, None),
        (220, 100, 48, 192, None), (300, 10, 20, 30, 0.2), (330, 10, 20, 30, 1 / 3), (360, 10, 20, 30, 1.0),
        (400, 10, 25, 25, 0.19999), (430, 300, 33, 33, 3.0),
    ]
    dets = []
    for n, (x, y, w, h, r) in enumerate(extra):
        a = {"id": nid + n, "image_id": img, "category_id": cats[n % 3], "bbox": [float(x), float(y), float(w), float(h)],
             "area": float(w * h), "iscrowd": 0}
        if r is not None:
            a["ratio"] = r
        ds["annotations"].append(a)
        dets.append((x, y, x + w, y + h, n % 3))
    # detections with w/h exactly at the range bounds 1/5, 1/3, 3 and 5, unmatched
    for n, (w, h) in enumerate([(10, 50), (10, 30), (30, 10), (50, 10), (10, 10)]):
        dets.append((500 + 20 * n, 400, 500 + 20 * n + w, 400 + h, n % 3))
    m = len(dets)
    pr["image_id"] = np.concatenate([pr["image_id"], np.full(m, img, np.int64)])
    pr["category"] = np.concatenate([pr["category"], np.array([d[4] for d in dets], np.int64)])
    pr["boxes"] = np.concatenate([pr["boxes"], np.array([d[:4] for d in dets], np.float32)])
    pr["score"] = np.concatenate([pr["score"], np.linspace(0.9, 0.3, m).astype(np.float32)])
    return ds, pr


def _case_truncation():
    return synthetic_coco(14, n_images=10, n_cats=2, dets_per_image=(60, 260), no_dt=0.0, max_gts=20)


def _case_degenerate():
    ds, pr = synthetic_coco(15, n_images=20, n_cats=4, dets_per_image=(0, 20), no_gt=0.0)
    cats = sorted(c["id"] for c in ds["categories"])
    only_crowd = ds["images"][3]["id"]
    for a in ds["annotations"]:
        if a["image_id"] == only_crowd or a["category_id"] == cats[1]:
            a["iscrowd"] = 1        # an image with only crowd gts; a category whose gts are all ignored in every range
        if a["category_id"] == cats[3]:
            a["ratio"] = 0.5        # a category whose gts are all ignored in the slender ranges
    return ds, pr


CASES = {"general": _case_general, "ties": _case_ties, "boundaries": _case_boundaries, "truncation": _case_truncation,
         "degenerate": _case_degenerate}


def pred_order(ds, pr):
    """Images in json order, each once: the order a loader would hand them to process()."""
    return np.array([im["id"] for im in ds["images"]], np.int64)


def d2_predictions(ds, pr, id_map, limit=None):
    """What detectron2's COCOEvaluator.process() keeps: per image, instances_to_coco_json (contiguous category ids)."""
    xywh = preds_xywh(pr)
    out = []
    for img in pred_order(ds, pr):
        sel = np.nonzero(pr["image_id"] == img)[0]
        if limit is not None:
            sel = sel[:limit]
        inst = [{"image_id": int(img), "category_id": int(pr["category"][i]), "bbox": [float(v) for v in xywh[i]],
                 "score": float(pr["score"][i])} for i in sel]
        out.append({"image_id": int(img), "instances": inst})
    return out


def run_case(mods, ds, pr):
    ce, co, ev = mods
    coco_api = co.COCO(copy.deepcopy(ds))
    cats = sorted(coco_api.getCatIds())
    id_map = {c: i for i, c in enumerate(cats)}
    names = [coco_api.cats[c]["name"] for c in cats]
    meta = _Meta(thing_dataset_id_to_contiguous_id=id_map, thing_classes=names)
    self_ = object.__new__(ev.COCOEvaluator)
    self_._coco_api, self_._metadata, self_._results = coco_api, meta, {}
    self_._logger = types.SimpleNamespace(warn=lambda *a: None, warning=lambda *a: None)
    # AR pass: the reference fails beyond 100 predictions per image (boxes truncated, classes not); fed the first 100
    preds100 = d2_predictions(ds, pr, id_map, limit=100)
    ev.COCOEvaluator._evaluate_predictions_ar(self_, preds100)
    ar = self_._results["ar"]
    st = ev._evaluate_predictions_ar(preds100, coco_api, meta, aspect_ratios=AR_RATIOS, areas=AR_AREAS, limit=100)
    # COCOeval pass on dataset category ids
    rev = {v: k for k, v in id_map.items()}
    res = [dict(r, category_id=rev[r["category_id"]]) for p in d2_predictions(ds, pr, id_map) for r in p["instances"]]
    coco_dt = coco_api.loadRes(copy.deepcopy(res))
    E = ce.COCOeval(coco_api, coco_dt, "bbox")
    E.evaluate()
    E.accumulate()
    E.summarize()
    bbox = ev.COCOEvaluator._derive_coco_results(self_, E, "bbox", class_names=names)
    ar_dict = {k: float(v) for k, v in ar.items() if k != "ar-stats"}
    gt_ratio = np.array([coco_api.anns[a["id"]]["ratio"] for a in ds["annotations"]], np.float64)
    return {
        "dataset_json": np.array(json.dumps(ds)), "pred_order": pred_order(ds, pr),
        "pred_image_id": pr["image_id"], "pred_category": pr["category"], "pred_boxes": pr["boxes"], "pred_score": pr["score"],
        "gt_ratio": gt_ratio,
        "precision": E.eval["precision"], "recall": E.eval["recall"], "scores": E.eval["scores"], "stats": np.asarray(E.stats, np.float64),
        "bbox_results_json": np.array(json.dumps(bbox)),
        "ar_recalls": st["recalls"].numpy(), "ar_ar": st["ar"].numpy(), "ar_mar": st["mar"].numpy(), "ar_num_pos": st["num_pos"].numpy(),
        "ar_thresholds": st["thresholds"].numpy(), "ar_results_json": np.array(json.dumps(ar_dict)),
    }


def main():
    import contextlib
    import io

    mods = install()
    meta = {}
    for name, fn in CASES.items():
        ds, pr = fn()
        with contextlib.redirect_stdout(io.StringIO()):
            out = run_case(mods, ds, pr)
        fname = f"coco_eval_{name}.npz"
        with open(os.path.join(OUT, fname), "wb") as f:
            np.savez_compressed(f, **out)
        meta[fname] = ("reference-Python x restated-op: slender_det/evaluation/cocoeval.py (whole) + coco.py:27-84 + "
                       "coco_evaluation.py:166-417 x restated " + RESTATED +
                       f"; case '{name}'; AR pass fed each image's first 100 predictions")
    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
