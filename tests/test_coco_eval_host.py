"""Slender-object COCO evaluation, host side (CPU): the restatement (tests/coco_eval_restated.py) against the fixtures the
reference's own evaluation produced (tests/golden/coco_eval/), the gt index and ratio rules, the result dicts, the drop-in names
and the distributed merge."""
import inspect
import json
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import coco_eval_restated as RS
from slenderobjdet_amd.evaluation.coco_gt import CocoGt, gt_ratio, polygon_ratio
from slenderobjdet_amd.evaluation.results import ar_results, derive_coco_results, summarize
from slenderobjdet_amd.evaluation.synthetic import preds_xywh

G = os.path.join(os.path.dirname(__file__), "golden", "coco_eval")
CASES = ["general", "ties", "boundaries", "truncation", "degenerate"]


def load_case(name):
    d = dict(np.load(os.path.join(G, f"coco_eval_{name}.npz")))
    d["dataset"] = json.loads(str(d["dataset_json"]))
    d["bbox_results"] = json.loads(str(d["bbox_results_json"]))
    d["ar_results"] = json.loads(str(d["ar_results_json"]))
    return d


def restated_inputs(d):
    gt = CocoGt(d["dataset"])
    gts = [dict(a, ratio=float(r)) for a, r in zip(gt.anns, gt.ratios)]
    xywh = preds_xywh({"boxes": d["pred_boxes"]})
    cats = gt.cat_ids
    dets = {"image_id": d["pred_image_id"], "category_id": np.array([cats[c] for c in d["pred_category"]], np.int64), "bbox": xywh,
            "score": d["pred_score"]}
    by_img = {}
    for a in gts:
        by_img.setdefault(a["image_id"], []).append(a)
    images = []
    for img in d["pred_order"]:
        sel = np.nonzero(d["pred_image_id"] == img)[0]
        images.append((int(img), xywh[sel], d["pred_category"][sel]))
    return gt, gts, dets, by_img, images


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]


def assert_ulp(a, b, ulps=1):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.all(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= ulps), (a, b)


def assert_results_equal(got, ref):
    assert list(got) == list(ref)
    for k in ref:
        if isinstance(ref[k], dict):
            assert_results_equal(got[k], ref[k])
        elif isinstance(ref[k], list):
            assert got[k] == ref[k], k
        elif math.isnan(ref[k]):
            assert math.isnan(got[k]), k
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference_fixture(case):
    d = load_case(case)
    gt, gts, dets, by_img, images = restated_inputs(d)
    np.testing.assert_array_equal(gt.ratios, d["gt_ratio"])
    precision, recall, scores = RS.match_and_accumulate(gt.img_ids, gt.cat_ids, gts, dets)
    _same(precision, d["precision"])
    _same(recall, d["recall"])
    _same(scores, d["scores"])
    stats = RS.summarize(precision, recall)
    _same(stats, d["stats"])
    assert_results_equal(RS.derive_bbox_results(stats, precision, [gt.cats[c]["name"] for c in gt.cat_ids]), d["bbox_results"])
    recalls, ar, mar, num_pos, _ = RS.proposal_ar(images, by_img, gt.id_map, len(gt.cat_ids))
    _same(recalls.numpy(), d["ar_recalls"])
    _same(num_pos.numpy(), d["ar_num_pos"])
    assert_ulp(ar.numpy(), d["ar_ar"])
    assert_ulp(mar.numpy(), d["ar_mar"])


@pytest.mark.parametrize("case", CASES)
def test_result_dicts_from_fixture_arrays(case):
    """The package's host summaries, fed the reference's arrays, give the reference's dicts: keys, order, values, NaN rules."""
    d = load_case(case)
    gt = CocoGt(d["dataset"])
    _same(summarize(d["precision"], d["recall"]), d["stats"])
    names = [gt.cats[c]["name"] for c in gt.cat_ids]
    assert_results_equal(derive_coco_results(d["stats"], d["precision"], names), d["bbox_results"])
    res = ar_results(torch.from_numpy(d["ar_recalls"]), torch.from_numpy(d["ar_num_pos"]))
    st = res.pop("ar-stats")
    assert_results_equal(res, d["ar_results"])
    assert list(st) == ["ar", "mar", "thresholds", "gt_overlaps", "num_pos"]
    _same(st["thresholds"].numpy(), d["ar_thresholds"])


def test_derive_results_nan_rules():
    stats = np.array([0.5, -1, 0.25, -1, 0.1, 0.0] + [-1] * 10)
    prec = -np.ones((10, 101, 1, 6, 3))
    r = derive_coco_results(stats, prec, ["only"])
    assert list(r) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]       # one class: no AP-ratios
    assert r["AP"] == 50.0 and math.isnan(r["AP50"]) and math.isnan(r["APs"]) and r["APl"] == 0.0
    assert all(math.isnan(v) for v in derive_coco_results(None, None).values())


def test_meta_labels_every_fixture():
    meta = json.load(open(os.path.join(G, "meta.json")))
    assert sorted(meta) == sorted(f for f in os.listdir(G) if f.endswith(".npz"))
    for v in meta.values():
        assert v.startswith("reference-Python x restated-op") and "pycocotools" in v and "detectron2" in v


def _rotated_rect(cx, cy, w, h, deg):
    t = math.radians(deg)
    c, s = math.cos(t), math.sin(t)
    pts = []
    for x, y in [(-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)]:
        pts += [cx + c * x - s * y, cy + s * x + c * y]
    return pts


@pytest.mark.parametrize("w,h,deg", [(10, 50, 0), (10, 50, 30), (30, 10, 45), (40, 40, 17), (7, 70, -62), (100, 1, 89)])
def test_polygon_ratio_on_rotated_rectangles(w, h, deg):
    pts = _rotated_rect(200, 150, w, h, deg)
    assert abs(polygon_ratio([pts]) - min(w, h) / max(w, h)) < 1e-6
    # extra interior points and a second polygon inside do not change the hull
    inner = _rotated_rect(200, 150, w / 3, h / 3, deg)
    assert abs(polygon_ratio([pts, inner]) - min(w, h) / max(w, h)) < 1e-6


def test_gt_ratio_rules():
    assert gt_ratio({"ratio": 0.7, "iscrowd": 0, "bbox": [0, 0, 10, 50]}) == 0.7                              # explicit wins
    assert gt_ratio({"iscrowd": 0, "bbox": [0, 0, 10, 50]}) == 10 / 50                                          # no segmentation
    assert gt_ratio({"iscrowd": 1, "bbox": [0, 0, 60, 20], "segmentation": [_rotated_rect(0, 0, 5, 50, 10)]}) == 20 / 60   # crowd
    assert gt_ratio({"iscrowd": 0, "bbox": [0, 0, 60, 20], "segmentation": [[1, 2, 3, 4]]}) == 20 / 60        # no usable polygon
    assert gt_ratio({"iscrowd": 0, "bbox": [0, 0, 60, 20], "segmentation": {"counts": "x", "size": [4, 4]}}) == 20 / 60   # RLE
    r = gt_ratio({"iscrowd": 0, "bbox": [0, 0, 60, 20], "segmentation": [_rotated_rect(50, 50, 8, 40, 33)]})
    assert abs(r - 0.2) < 1e-6
    # a hull of fewer than 3 points falls back to the axis-aligned extent of the points
    assert gt_ratio({"iscrowd": 0, "bbox": [0, 0, 1, 1], "segmentation": [[0, 0, 5, 5, 10, 10]]}) == 1.0
    assert gt_ratio({"iscrowd": 0, "bbox": [0, 0, 1, 1], "segmentation": [[0, 0, 0, 5, 0, 10]]}) == 0.0


def test_gt_index_and_category_maps():
    ds = {"images": [{"id": 9}, {"id": 2}], "categories": [{"id": 7, "name": "b"}, {"id": 3, "name": "a"}],
          "annotations": [{"id": 1, "image_id": 9, "category_id": 7, "bbox": [0, 0, 4, 2], "iscrowd": 0},
                          {"id": 2, "image_id": 2, "category_id": 3, "bbox": [0, 0, 4, 4], "iscrowd": 1},
                          {"id": 3, "image_id": 9, "category_id": 7, "bbox": [1, 1, 2, 8], "iscrowd": 0, "ratio": 0.3}]}
    gt = CocoGt(ds)
    assert gt.img_ids == [2, 9] and gt.cat_ids == [3, 7] and gt.id_map == {3: 0, 7: 1}
    h = gt.arrays()
    # segments (k, i): (3, 2) holds ann 2; (7, 9) holds anns 1 and 3 in json order
    assert h["seg_gt_off"].tolist() == [0, 1, 1, 1, 3]
    assert h["seg_ratio"].tolist() == [1.0, 0.5, 0.3] and h["seg_crowd"].tolist() == [1, 0, 0]
    assert h["img_gt_off"].tolist() == [0, 0, 2] and h["img_cls"].tolist() == [1, 1]       # the crowd gt is not in the recall pass
    gt2 = CocoGt(ds, id_map={3: 1, 7: 0}, class_names=["b", "a"])
    assert gt2.arrays()["img_cls"].tolist() == [0, 0] and gt2.class_names == ["b", "a"]


def test_dropin_binds_the_evaluation():
    import slenderobjdet_amd.dropin  # noqa: F401
    import detectron2.evaluation as d2e
    import slender_det.evaluation as se
    from slenderobjdet_amd import evaluation as ev

    assert se.COCOEvaluator is ev.COCOEvaluator and d2e.COCOEvaluator is ev.COCOEvaluator
    assert d2e.DatasetEvaluator is ev.DatasetEvaluator and d2e.DatasetEvaluators is ev.DatasetEvaluators
    assert se.inference_on_dataset is ev.inference_on_dataset
    assert list(inspect.signature(se.inference_on_dataset).parameters) == ["dataset_name", "model", "data_loader", "evaluator"]
    assert list(inspect.signature(ev.COCOEvaluator).parameters) == ["dataset_name", "cfg", "distributed", "output_dir"]
    with pytest.raises(NotImplementedError):
        d2e.RotatedCOCOEvaluator("x")


def test_non_bbox_tasks_raise(tmp_path):
    from types import SimpleNamespace

    from slenderobjdet_amd.data.catalog import MetadataCatalog
    from slenderobjdet_amd.evaluation import COCOEvaluator

    p = tmp_path / "gt.json"
    p.write_text(json.dumps({"images": [], "annotations": [], "categories": []}))
    MetadataCatalog.get("host_tasks").json_file = str(p)
    COCOEvaluator("host_tasks", SimpleNamespace(MODEL=SimpleNamespace(MASK_ON=False)), False)
    with pytest.raises(NotImplementedError):
        COCOEvaluator("host_tasks", SimpleNamespace(MODEL=SimpleNamespace(MASK_ON=True)), False)


def _fake_outputs(preds, images):
    from slenderobjdet_amd.structures import Boxes, Instances

    inputs, outputs = [], []
    for img in images:
        sel = np.nonzero(preds["image_id"] == img)[0]
        inst = Instances((480, 640))
        inst.pred_boxes = Boxes(torch.from_numpy(preds["boxes"][sel]))
        inst.scores = torch.from_numpy(preds["score"][sel])
        inst.pred_classes = torch.from_numpy(preds["category"][sel])
        inputs.append({"image_id": int(img)})
        outputs.append({"instances": inst})
    return inputs, outputs


def _ddp_worker(rank, world, store, json_file, out_file):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world)
    try:
        from slenderobjdet_amd.data.catalog import MetadataCatalog
        from slenderobjdet_amd.evaluation import COCOEvaluator

        d = load_case("general")
        MetadataCatalog.get("ddp_merge").json_file = json_file
        ev = COCOEvaluator("ddp_merge", None, True)
        imgs = list(d["pred_order"])
        half = (len(imgs) + 1) // 2
        mine = imgs[:half] if rank == 0 else imgs[half:]
        preds = {"image_id": d["pred_image_id"], "boxes": d["pred_boxes"], "score": d["pred_score"], "category": d["pred_category"]}
        ev.process(*_fake_outputs(preds, mine))
        n, flat = ev._gather()
        if rank == 0:
            torch.save((n, flat), out_file)
        else:
            assert flat is None and n == 0
    finally:
        dist.destroy_process_group()


def test_distributed_merge_equals_single_process(tmp_path):
    import torch.multiprocessing as mp

    from slenderobjdet_amd.data.catalog import MetadataCatalog
    from slenderobjdet_amd.evaluation import COCOEvaluator

    d = load_case("general")
    jf = tmp_path / "gt.json"
    jf.write_text(json.dumps(d["dataset"]))
    out = str(tmp_path / "merged.pt")
    mp.spawn(_ddp_worker, args=(2, str(tmp_path / "store"), str(jf), out), nprocs=2, join=True)
    n2, flat2 = torch.load(out)
    MetadataCatalog.get("ddp_single").json_file = str(jf)
    ev = COCOEvaluator("ddp_single", None, False)
    preds = {"image_id": d["pred_image_id"], "boxes": d["pred_boxes"], "score": d["pred_score"], "category": d["pred_category"]}
    ev.process(*_fake_outputs(preds, list(d["pred_order"])))
    n1, flat1 = ev._gather()
    assert n1 == n2 == len(d["pred_order"])
    assert list(flat1) == list(flat2)
    for k in flat1:
        assert torch.equal(flat1[k], flat2[k]), k
