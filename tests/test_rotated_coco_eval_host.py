"""Rotated-box COCO evaluation, host side (CPU): the public surface, the gt arrays of CocoGt.rotated_arrays(), the result dicts,
the restatement (tests/rotated_coco_eval_restated.py) on cases whose answer is known without any program, the drop-in opt-in and
the C ABI's declaration."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rotated_coco_eval_restated as RR
from test_coco_eval_host import _same, assert_results_equal

from slenderobjdet_amd.evaluation.coco_gt import CocoGt
from slenderobjdet_amd.evaluation.results import derive_ratio_results, derive_rotated_results, summarize_area

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ hand-derived cases
def _dataset(boxes_by_image, cats=(1,)):
    """boxes_by_image: {image_id: [(category_id, bbox), ...]}; area = w * h."""
    images, anns = [], []
    for img, items in boxes_by_image.items():
        images.append({"id": img, "width": 640, "height": 480})
        for c, b in items:
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": c, "bbox": list(b), "area": float(b[2] * b[3]), "iscrowd": 0})
    return {"images": images, "annotations": anns, "categories": [{"id": c, "name": f"c{c}"} for c in cats]}


def _preds(rows):
    """rows: (image_id, contiguous category, box, score)."""
    return {"image_id": np.array([r[0] for r in rows], np.int64), "category": np.array([r[1] for r in rows], np.int64),
            "boxes": np.array([r[2] for r in rows], np.float32).reshape(len(rows), len(rows[0][2]) if rows else 5), "score": np.array([r[3] for r in rows], np.float32)}


# well separated boxes (no two of one image overlap), two categories, three images
PERFECT_GTS = {
    11: [(1, (100.0, 100.0, 60.0, 20.0, 30.0)), (1, (300.0, 120.0, 40.0, 40.0, -20.0)), (3, (480.0, 300.0, 150.0, 30.0, 75.0))],
    12: [(3, (200.0, 200.0, 24.0, 18.0, 0.0)), (1, (420.0, 90.0, 90.0, 12.0, -60.0))],
    13: [(1, (320.0, 240.0, 200.0, 110.0, 45.0))],
}


def case_perfect(swapped=False):
    """Every gt predicted exactly (score 1); ``swapped``: as (cx, cy, h, w, angle + 90), the same region of the plane."""
    ds = _dataset(PERFECT_GTS, cats=(1, 3))
    contig = {1: 0, 3: 1}
    rows = []
    for img, items in PERFECT_GTS.items():
        for c, (cx, cy, w, h, ang) in items:
            rows.append((img, contig[c], (cx, cy, h, w, ang + 90.0) if swapped else (cx, cy, w, h, ang), 1.0))
    return ds, _preds(rows)


def case_squares():
    """One gt, one detection: concentric 10 x 10 squares 45 degrees apart.  The intersection is a regular octagon of area
    200 (sqrt 2 - 1), the union 200 - that: IoU = (2 sqrt 2 - 2) / (4 - 2 sqrt 2) = 0.70710..., so the detection matches at the
    thresholds .5 .. .70 and not from .75 up."""
    ds = _dataset({5: [(1, (50.0, 50.0, 10.0, 10.0, 0.0))]})
    return ds, _preds([(5, 0, (50.0, 50.0, 10.0, 10.0, 45.0), 0.9)])


def case_area_buckets():
    """One gt per area bucket (20 x 20 small, 50 x 50 medium, 120 x 120 large) with an exact detection on each."""
    boxes = [(100.0, 100.0, 20.0, 20.0, 15.0), (300.0, 100.0, 50.0, 50.0, -30.0), (300.0, 320.0, 120.0, 120.0, 60.0)]
    ds = _dataset({7: [(1, b) for b in boxes]})
    return ds, _preds([(7, 0, b, s) for b, s in zip(boxes, (0.9, 0.8, 0.7))])


def restated_eval(ds, preds, bucket="area", iou_fn=RR.oracle_iou):
    img_ids, cat_ids, gts, dets = RR.restated_inputs(ds, preds, bucket)
    ranges = RR.AREA_RNG if bucket == "area" else RR.RATIO_RNG
    return RR.match_and_accumulate(img_ids, cat_ids, gts, dets, ranges, iou_fn)


def _eq(x, want):
    """Equal up to the 2^-52 that COCOeval.accumulate adds to every precision denominator (tp / (fp + tp + eps))."""
    return abs(x - want) <= 1e-12 * max(abs(want), 1.0)


def check_perfect(stats, res):
    assert all(_eq(stats[i], 1.0) for i in (0, 1, 2)) and stats[8] == 1.0     # AP, AP50, AP75, AR@100
    assert all(_eq(res[k], 100.0) for k in ("AP", "AP50", "AP75", "AP-c1", "AP-c3"))


def check_squares(recall, stats, res):
    assert recall[:, 0, 0, 2].tolist() == [1.0] * 5 + [0.0] * 5               # matched at .50 .. .70 only
    assert _eq(stats[0], 0.5) and _eq(stats[1], 1.0) and stats[2] == 0.0 and stats[8] == 0.5
    assert _eq(stats[3], 0.5) and stats[4] == -1 and stats[5] == -1           # area 100: the small bucket
    assert _eq(res["AP"], 50.0) and _eq(res["AP50"], 100.0) and res["AP75"] == 0.0 and math.isnan(res["APm"]) and math.isnan(res["APl"])


def check_area_buckets(stats, res):
    assert all(_eq(res[k], 100.0) for k in ("AP", "APs", "APm", "APl"))
    assert stats[9] == stats[10] == stats[11] == 1.0                          # AR small / medium / large
    assert _eq(stats[6], 1.0 / 3.0)                                           # AR@1: one of the three gts


# ------------------------------------------------------------------------------------------------ surface
def test_public_surface():
    from slenderobjdet_amd import evaluation as ev
    from slenderobjdet_amd.evaluation import COCOEvaluator, RotatedCOCOEvaluator

    assert issubclass(RotatedCOCOEvaluator, COCOEvaluator) and "RotatedCOCOEvaluator" in ev.__all__
    assert list(inspect.signature(RotatedCOCOEvaluator).parameters) == ["dataset_name", "cfg", "distributed", "output_dir", "ratio_buckets"]
    assert inspect.signature(RotatedCOCOEvaluator).parameters["ratio_buckets"].default is False
    # process / reset / _gather are the base class's
    assert RotatedCOCOEvaluator.process is COCOEvaluator.process and RotatedCOCOEvaluator._gather is COCOEvaluator._gather
    assert RotatedCOCOEvaluator.reset is COCOEvaluator.reset


def test_cabi_declares_the_rotated_pass():
    from slenderobjdet_amd import _C
    from test_cabi_surface import _declared

    decl = _declared()
    assert decl["sod_coco_match_rotated_scratch_floats"] == 2 == len(_C._SIGS["sod_coco_match_rotated_scratch_floats"])
    assert decl["sod_coco_match_rotated"] == 20 == len(_C._SIGS["sod_coco_match_rotated"])
    import ctypes

    assert _C._RESTYPES["sod_coco_match_rotated_scratch_floats"] is ctypes.c_longlong
    text = open(os.path.join(ROOT, "include", "slender_hip.h")).read()
    assert "train_net.py:60-62" in text and "RotatedCOCOeval.computeIoU" in text


def test_scratch_size_query():
    from slenderobjdet_amd import _C

    lib = _C.load()
    q = lib.sod_coco_match_rotated_scratch_floats
    assert q(0, 100) == 0 and q(32, 100) == 0 and q(-1, 100) == -1
    assert q(33, 100) == 3300                                  # 33 * 100 > 3200 floats: the IoU matrix alone
    assert q(65, 100) == 6500 + 2 * 64 * 2                     # plus 64 lanes x 2 words of matched-gt bits
    assert q(33, 101) == 3334                                  # the IoU part is kept even (8-byte aligned bit rows behind it)


# ------------------------------------------------------------------------------------------------ gt arrays
def _four_ann_dataset():
    return {"images": [{"id": 9}, {"id": 2}], "categories": [{"id": 7, "name": "b"}, {"id": 3, "name": "a"}],
            "annotations": [
                {"id": 1, "image_id": 9, "category_id": 7, "bbox": [50.5, 40.25, 30.0, 10.0, -35.0], "area": 280.0, "iscrowd": 0},
                {"id": 2, "image_id": 2, "category_id": 3, "bbox": [10.1, 20.2, 4.4, 8.6], "iscrowd": 0},
                {"id": 3, "image_id": 9, "category_id": 7, "bbox": [1.0, 1.0, 2.0, 8.0], "area": 15.5, "iscrowd": 0, "ratio": 0.3},
                {"id": 4, "image_id": 2, "category_id": 7, "bbox": [100.0, 100.0, 80.0, 20.0, 90.0], "iscrowd": 0}]}


def test_rotated_arrays():
    ds = _four_ann_dataset()
    gt = CocoGt(ds)
    h = gt.rotated_arrays()
    assert list(h) == ["seg_gt_off", "seg_box5", "seg_crowd", "seg_area", "seg_ratio5"]
    # segments (k, i) over cat_ids [3, 7] x img_ids [2, 9]: (3, 2) ann 2; (7, 2) ann 4; (7, 9) anns 1 and 3 in json order
    assert h["seg_gt_off"].tolist() == [0, 1, 1, 2, 4] and np.array_equal(h["seg_gt_off"], gt.arrays()["seg_gt_off"])
    assert h["seg_box5"].dtype == np.float32 and h["seg_box5"].shape == (4, 5)
    f = np.float32
    xywh = np.array([10.1, 20.2, 4.4, 8.6], f)
    want = [[xywh[0] + xywh[2] / f(2), xywh[1] + xywh[3] / f(2), xywh[2], xywh[3], 0.0],
            [100.0, 100.0, 80.0, 20.0, 90.0], [50.5, 40.25, 30.0, 10.0, -35.0], [2.0, 5.0, 2.0, 8.0, 0.0]]
    _same(h["seg_box5"], np.array(want, f))
    assert h["seg_area"].dtype == np.float64 and h["seg_area"].tolist() == [4.4 * 8.6, 80.0 * 20.0, 280.0, 15.5]
    assert h["seg_ratio5"].tolist() == [4.4 / 8.6, 20.0 / 80.0, 10.0 / 30.0, 0.3]
    assert h["seg_crowd"].dtype == np.uint8 and h["seg_crowd"].tolist() == [0, 0, 0, 0]
    assert gt.rotated_arrays() is h
    # the axis-aligned arrays are untouched by the rotated ones
    assert gt.arrays()["seg_ratio"].tolist() == [4.4 / 8.6, 20.0 / 80.0, 10.0 / 30.0, 0.3]
    # the restatement's own conversion agrees
    _, _, gts, _ = RR.restated_inputs(ds, _preds([]))
    by_id = {g["id"]: g for g in gts}
    _same(np.stack([by_id[i]["box5"] for i in (2, 4, 1, 3)]), h["seg_box5"])
    assert [by_id[i]["val"] for i in (2, 4, 1, 3)] == h["seg_area"].tolist()


def test_rotated_arrays_refuse_crowd_beside_rotated_boxes():
    ds = _four_ann_dataset()
    ds["annotations"][1]["iscrowd"] = 1
    with pytest.raises(ValueError):
        CocoGt(ds).rotated_arrays()
    # crowd gts among XYWH boxes only are fine (and flagged)
    for a in ds["annotations"]:
        a["bbox"] = a["bbox"][:4]
    assert CocoGt(ds).rotated_arrays()["seg_crowd"].tolist() == [1, 0, 0, 0]


def test_evaluator_refuses_crowd_beside_rotated_boxes(tmp_path):
    import json

    from slenderobjdet_amd.data.catalog import MetadataCatalog
    from slenderobjdet_amd.evaluation import RotatedCOCOEvaluator

    ds = _four_ann_dataset()
    p = tmp_path / "ok.json"
    p.write_text(json.dumps(ds))
    MetadataCatalog.get("rot_host_ok").json_file = str(p)
    RotatedCOCOEvaluator("rot_host_ok", None, False)
    ds["annotations"][1]["iscrowd"] = 1
    p = tmp_path / "crowd.json"
    p.write_text(json.dumps(ds))
    MetadataCatalog.get("rot_host_crowd").json_file = str(p)
    with pytest.raises(ValueError):
        RotatedCOCOEvaluator("rot_host_crowd", None, False)


# ------------------------------------------------------------------------------------------------ result dicts
def test_summaries_equal_restatement_on_hand_filled_arrays():
    rs = np.random.RandomState(3)
    T, R, K, A, M = 10, 101, 3, 4, 3
    precision = rs.rand(T, R, K, A, M)
    recall = rs.rand(T, K, A, M)
    precision[:, :, 1] = -1                      # a category without gts
    recall[:, 1] = -1
    precision[:, :, :, 3] = -1                   # no large gt at all
    recall[:, :, 3] = -1
    stats = summarize_area(precision, recall)
    assert stats.shape == (12,)
    _same(stats, RR.summarize_area(precision, recall))
    assert stats[5] == -1 and stats[11] == -1
    assert _eq(stats[0], np.mean(precision[:, :, [0, 2], 0, 2])) and _eq(stats[6], np.mean(recall[:, [0, 2], 0, 0]))
    assert _eq(stats[1], np.mean(precision[0, :, [0, 2], 0, 2])) and _eq(stats[2], np.mean(precision[5, :, [0, 2], 0, 2]))
    assert _eq(stats[4], np.mean(precision[:, :, [0, 2], 2, 2])) and _eq(stats[10], np.mean(recall[:, [0, 2], 2, 2]))
    names = ["a", "b", "c"]
    res = derive_rotated_results(stats, precision, names)
    assert_results_equal(res, RR.derive_results(stats, precision, names))
    assert list(res) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-a", "AP-b", "AP-c"]
    assert res["AP"] == float(stats[0] * 100) and math.isnan(res["APl"]) and math.isnan(res["AP-b"])
    assert _eq(res["AP-c"], float(np.mean(precision[:, :, 2, 0, -1]) * 100))
    assert list(derive_rotated_results(stats, precision, ["only"])) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    none = derive_rotated_results(None, None, names)
    assert list(none) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and all(math.isnan(v) for v in none.values())
    assert_results_equal(none, RR.derive_results(None, None, names))


def test_ratio_result_dict():
    stats = np.array([0.5, -1, 0.25] + [0.1, -1, 0.3, 0.4, 0.0] + [0.2, 0.3, 0.4] + [-1, 0.6, 0.7, 0.8, 0.9])
    res = derive_ratio_results(stats)
    assert_results_equal(res, RR.derive_ratio_results(stats))
    assert len(res) == 16 and list(res)[:4] == ["AP", "AP50", "AP75", "AP- 0  - 1/5"] and list(res)[8:12] == ["AR@1", "AR@10", "AR@100", "AR- 0  - 1/5"]
    assert res["AP"] == 50.0 and math.isnan(res["AP50"]) and res["AP-5/1 - INF"] == 0.0 and math.isnan(res["AR- 0  - 1/5"])
    assert all(math.isnan(v) for v in derive_ratio_results(None).values())


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_perfect_predictor_and_swapped_description():
    out = []
    for swapped in (False, True):
        ds, preds = case_perfect(swapped)
        precision, recall, scores = restated_eval(ds, preds)
        stats = RR.summarize_area(precision, recall)
        check_perfect(stats, RR.derive_results(stats, precision, ["c1", "c3"]))
        out.append((precision, recall, scores, stats))
    for a, b in zip(*out):                                   # the same regions: the same result
        _same(a, b)


def test_restatement_concentric_squares():
    ds, preds = case_squares()
    iou = RR.oracle_iou(preds["boxes"], np.array([ds["annotations"][0]["bbox"]], np.float32))
    assert abs(float(iou[0, 0]) - (2 * math.sqrt(2) - 2) / (4 - 2 * math.sqrt(2))) < 1e-5
    precision, recall, _ = restated_eval(ds, preds)
    stats = RR.summarize_area(precision, recall)
    check_squares(recall, stats, RR.derive_results(stats, precision, ["c1"]))


def test_restatement_one_gt_per_area_bucket():
    ds, preds = case_area_buckets()
    precision, recall, _ = restated_eval(ds, preds)
    stats = RR.summarize_area(precision, recall)
    check_area_buckets(stats, RR.derive_results(stats, precision, ["c1"]))


def test_restatement_scan_rules():
    """Float32 comparison, ties to the later gt, ignored gts last and only while no real gt matched, crowd gts matched again."""
    f = np.float32
    rng = [[0, 1e10], [0, 100]]
    # the float32 of 0.7 is below the float64 0.7: in float32 the IoU equals the bound and matches (pycocotools in float64 would not)
    mt, ig, npig = RR.match_segment(np.array([[f(0.7)]], f), [0], [50.0], [50.0], rng)
    assert mt[4, 0, 0] and not mt[5, 0, 0] and npig.tolist() == [1, 1]
    # a tie goes to the later gt; the second detection then takes the earlier one
    mt, ig, _ = RR.match_segment(np.array([[0.8, 0.8], [0.8, 0.8], [0.8, 0.8]], f), [0, 0], [50.0, 50.0], [50.0, 50.0, 50.0], rng)
    assert mt[0, 0].tolist() == [True, True, False]
    # range 1 ignores gt 1 (val 500): the detection prefers the real gt 0 although gt 1 overlaps more; alone it matches the ignored gt
    mt, ig, npig = RR.match_segment(np.array([[0.6, 0.9]], f), [0, 0], [50.0, 500.0], [50.0], rng)
    assert mt[0, 1, 0] and not ig[0, 1, 0] and npig.tolist() == [2, 1]
    mt, ig, _ = RR.match_segment(np.array([[0.1, 0.9]], f), [0, 0], [50.0, 500.0], [50.0], rng)
    assert mt[0, 1, 0] and ig[0, 1, 0] and mt[0, 0, 0] and not ig[0, 0, 0]
    # an unmatched detection outside the range is ignored, inside it is a false positive
    mt, ig, _ = RR.match_segment(np.array([[0.1]], f), [0], [50.0], [500.0], rng)
    assert not mt[0, 1, 0] and ig[0, 1, 0] and not ig[0, 0, 0]
    # a crowd gt is ignored and can be matched by both detections
    mt, ig, npig = RR.match_segment(np.array([[0.9], [0.9]], f), [1], [50.0], [50.0, 50.0], rng)
    assert mt[0, 0].tolist() == [True, True] and ig[0, 0].tolist() == [True, True] and npig.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ drop-in
def test_bind_rotated_evaluator_in_a_child_interpreter():
    """The opt-in rebinds detectron2.evaluation.RotatedCOCOEvaluator; importing the drop-in alone keeps the stub.  Run in a child
    so that the rebinding does not outlive the test."""
    code = (
        "import slenderobjdet_amd.dropin as dropin\n"
        "import detectron2.evaluation as d2e\n"
        "from slenderobjdet_amd.evaluation import RotatedCOCOEvaluator\n"
        "assert d2e.RotatedCOCOEvaluator is not RotatedCOCOEvaluator\n"
        "try:\n"
        "    d2e.RotatedCOCOEvaluator('x')\n"
        "    raise SystemExit('the stub did not raise')\n"
        "except NotImplementedError:\n"
        "    pass\n"
        "assert dropin.bind_rotated_evaluator() is RotatedCOCOEvaluator\n"
        "assert d2e.RotatedCOCOEvaluator is RotatedCOCOEvaluator\n"
        "from detectron2.evaluation import RotatedCOCOEvaluator as again, COCOEvaluator\n"
        "assert again is RotatedCOCOEvaluator and issubclass(again, COCOEvaluator)\n"
        "print('bound')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("bound"), out.stdout + out.stderr


def test_synthetic_rotated_coco_recipe():
    from slenderobjdet_amd.evaluation.synthetic import synthetic_rotated_coco

    ds, preds = synthetic_rotated_coco(5, n_images=30, n_cats=4, dets_per_image=(0, 12))
    ds2, preds2 = synthetic_rotated_coco(5, n_images=30, n_cats=4, dets_per_image=(0, 12))
    assert ds == ds2 and all(np.array_equal(preds[k], preds2[k]) for k in preds)
    assert preds["boxes"].dtype == np.float32 and preds["boxes"].shape == (len(preds["score"]), 5) and len(preds["score"]) > 0
    assert all(len(a["bbox"]) == 5 and a["iscrowd"] == 0 and a["area"] == a["bbox"][2] * a["bbox"][3] for a in ds["annotations"])
    ang = np.array([a["bbox"][4] for a in ds["annotations"]])
    assert ang.min() >= -90 and ang.max() <= 90 and ang.std() > 20
    CocoGt(ds).rotated_arrays()
