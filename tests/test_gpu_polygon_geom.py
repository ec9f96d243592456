"""csrc/polygon_geom.hip on the GPU: minimum-area rectangles of polygons against the float64 restatement (polygon_geom_restated.py),
against the numpy path, around the LDS slice, on inputs that try the bounds of its loops, and through its consumers."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import polygon_geom_restated as R
from test_polygon_geom_host import _rect_dataset

from slenderobjdet_amd.data.catalog import MetadataCatalog
from slenderobjdet_amd.evaluation import COCOEvaluator, RotatedCOCOEvaluator
from slenderobjdet_amd.evaluation.coco_evaluation import predictions_from_numpy
from slenderobjdet_amd.evaluation.coco_gt import CocoGt
from slenderobjdet_amd.structures.polygons import LDS_POINTS, min_area_rects, pack_polygons

pytestmark = pytest.mark.gpu


def _launch(pts_list, device):
    xy = np.concatenate(pts_list) if pts_list else np.zeros((0, 2))
    off = np.cumsum([0] + [len(p) for p in pts_list])
    return min_area_rects(xy, off, device)


@pytest.fixture(scope="module")
def generated(cuda):
    """The 4 000 generated annotations, their oracle results, and the GPU's and the numpy path's answers (one launch)."""
    polys, pts, oracle = R.generated_with_oracle(4000)
    xy, off, index = pack_polygons(R.as_annotations(polys))
    assert len(index) == 4000
    gpu = min_area_rects(xy, off, cuda)
    cpu = min_area_rects(xy, off, "cpu")
    return pts, oracle, gpu, cpu


def test_parity_with_restatement(generated):
    """Left out of the five-number comparison by the oracle alone: 33 of 4 000 = 0.83 % (29 triangles, 4 quadrilaterals; none for
    the fold at 45).  Every annotation is checked for enclosure, least area and hull size."""
    pts, oracle, (rect, info), _ = generated
    assert rect.dtype == np.float64 and info.dtype == np.int32
    left_out = R.check_parity(pts, oracle, rect, info)
    print("left out of the full comparison:", left_out, "of", len(pts))


def test_gpu_and_numpy_paths_agree(generated):
    pts, oracle, (rect, info), (rect_np, info_np) = generated
    R.check_parity(pts, oracle, rect, info, ref_rect=rect_np)
    R.check_parity(pts, oracle, rect_np, info_np)
    print("largest difference of the two paths outside ties:",
          max(np.abs(a - b).max() for a, b, o in zip(rect, rect_np, oracle) if not R.is_tie(o[2])))


def test_sizes_around_the_lds_slice(cuda):
    rs = np.random.RandomState(5)
    C = LDS_POINTS
    sets = [np.round(rs.rand(n, 2) * (600, 400) + rs.rand(2) * 40, 2) for n in (C - 1, C, C + 1, 4 * C + 3)]
    t = rs.rand(50000) * 2 * math.pi
    r = 1 + 0.01 * rs.randn(50000)
    ellipse = np.stack([320 + 300 * r * np.cos(t), 240 + 90 * r * np.sin(t)], axis=1)
    c, s = math.cos(0.4), math.sin(0.4)
    sets.append(np.round(ellipse @ np.array([[c, s], [-s, c]]), 2))
    # a small annotation behind every large one: its slice is filled after the global-memory path ran in the same wave's block
    sets += [sets[0][:7], sets[1][:64], sets[2][:65]]
    oracle = [R.min_area_rect(p) for p in sets]
    rect, info = _launch(sets, cuda)
    R.check_parity(sets, oracle, rect, info, cap=None)
    assert all(o[1] >= 3 for o in oracle) and oracle[4][1] > 20


def test_no_annotation_and_one(cuda):
    from slenderobjdet_amd import _C

    rect, info = min_area_rects(np.zeros((0, 2)), [0], cuda)
    assert rect.shape == (0, 5) and rect.dtype == np.float64 and info.shape == (0,) and info.dtype == np.int32
    assert _C.load().sod_polygon_min_area_rect(None, None, 0, None, None, None) == 0       # A == 0 launches nothing
    assert _C.load().sod_polygon_min_area_rect(None, None, -1, None, None, None) == -1
    assert _C.load().sod_polygon_min_area_rect(None, None, (1 << 24) + 1, None, None, None) == -1
    pts = np.array([(10.0, 10.0), (90.0, 14.0), (130.0, 40.0), (118.0, 71.0), (40.0, 80.0), (5.0, 45.0)])
    rect, info = _launch([pts], cuda)
    R.check_parity([pts], [R.min_area_rect(pts)], rect, info, cap=0)


def test_4096_triangles(cuda):
    """One triangle per annotation: two annotations per wave, 512 blocks - every wave strides once.  Acute triangles are three-way
    ties and are compared by area, enclosure and hull size only."""
    rs = np.random.RandomState(6)
    tris = list(np.round(rs.rand(4096, 3, 2) * (640, 480), 2))
    oracle = [R.min_area_rect(p) for p in tris]
    rect, info = _launch(tris, cuda)
    left_out = R.check_parity(tris, oracle, rect, info, cap=None)
    assert 0 < left_out < 4096 * 0.5
    last = _launch(tris[:4093], cuda)                       # a last block with one wave at work
    assert np.array_equal(last[0], rect[:4093]) and np.array_equal(last[1], info[:4093])


def _bounded_inputs():
    rs = np.random.RandomState(7)
    t = np.arange(512) * (2 * math.pi / 512)
    circle = np.stack([300 + 200 * np.cos(t), 250 + 200 * np.sin(t)], axis=1)          # every point on the hull
    line = np.stack([np.arange(512.0), 0.5 * np.arange(512.0) + 1e-13 * rs.rand(512)], axis=1)
    quad = np.array([(10.0, 10.0), (90.0, 14.0), (118.0, 71.0), (5.0, 45.0)])
    copies = np.tile(quad, (300, 1))
    far = np.round(rs.rand(100, 2) * (640, 480), 2) + 1e6
    return {"circle": circle, "jittered_line": line, "copies": copies, "offset_1e6": far}


@pytest.mark.parametrize("name", ["circle", "jittered_line", "copies", "offset_1e6"])
def test_inputs_that_try_the_loop_bounds(cuda, name):
    """Each is one launch that has to come back: the hull walk stops after n steps whatever its orientation tests say.  The result
    is held to the oracle's area and to enclosure (the least area of the jittered line is rounding noise: side tolerance)."""
    pts = _bounded_inputs()[name]
    oracle = R.min_area_rect(pts)
    rect, info = _launch([pts], cuda)
    print(name, rect[0].tolist(), int(info[0]), "oracle", oracle[0], oracle[1])
    scale = max(1.0, float(np.abs(pts).max()))
    assert np.isfinite(rect).all() and 1 <= info[0] <= len(pts)
    assert R.encloses(rect[0], pts, 1e-9 * scale)
    area = oracle[2][0][0] if oracle[2] else oracle[0][2] * oracle[0][3]
    assert abs(rect[0, 2] * rect[0, 3] - area) <= 1e-9 * area + (oracle[0][2] + oracle[0][3]) * 1e-9 * scale
    if name == "copies":
        assert info[0] == 4


def test_rotated_gt_from_polygons_feeds_the_rotated_evaluator(cuda, tmp_path):
    from slenderobjdet_amd.data import coco_to_rotated

    ds, rects = _rect_dataset()
    out = coco_to_rotated(ds, skip_crowd=True, device="cuda")
    host = coco_to_rotated(ds, skip_crowd=True, device="cpu")
    for a, b in zip(out["annotations"], host["annotations"]):
        assert np.abs(np.array(a["bbox"]) - np.array(b["bbox"])).max() <= 1e-9
    jf = tmp_path / "rbox.json"
    jf.write_text(json.dumps(out))
    meta = MetadataCatalog.get("polygon_geom_rbox_gpu")
    meta.clear()
    meta.update(name="polygon_geom_rbox_gpu", json_file=str(jf))
    ev = RotatedCOCOEvaluator("polygon_geom_rbox_gpu", None, False)
    anns = out["annotations"]
    preds = {"image_id": np.array([a["image_id"] for a in anns], np.int64), "category": np.zeros(len(anns), np.int64),
             "boxes": np.array([a["bbox"] for a in anns], np.float32), "score": np.ones(len(anns), np.float32)}
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    assert res["bbox"]["AP"] == pytest.approx(100.0) and res["bbox"]["AP50"] == pytest.approx(100.0)


def test_evaluator_with_device_ratios_equals_the_default(cuda, tmp_path):
    """The synthetic evaluation set has bbox-only gts: both paths take the bbox rule.  This pins the plumbing, not the geometry."""
    from slenderobjdet_amd.evaluation.synthetic import synthetic_coco
    from test_coco_eval_host import assert_results_equal

    ds, preds = synthetic_coco(3)
    jf = tmp_path / "gt.json"
    jf.write_text(json.dumps(ds))
    gt = CocoGt(ds)
    meta = MetadataCatalog.get("polygon_geom_ratio_device")
    meta.clear()
    meta.update(name="polygon_geom_ratio_device", json_file=str(jf), thing_dataset_id_to_contiguous_id=dict(gt.id_map))
    flat = predictions_from_numpy(preds, cuda)
    ref = COCOEvaluator("polygon_geom_ratio_device", None, False).evaluate_flat(flat)
    meta["ratio_device"] = "cuda"          # the evaluator's constructor keeps the reference's four parameters: the option is metadata
    ev = COCOEvaluator("polygon_geom_ratio_device", None, False)
    assert np.array_equal(ev._gt.ratios, gt.ratios)
    got = ev.evaluate_flat(flat)
    assert list(got) == list(ref)
    assert_results_equal(got["bbox"], ref["bbox"])
    assert_results_equal({k: v for k, v in got["ar"].items() if k != "ar-stats"}, {k: v for k, v in ref["ar"].items() if k != "ar-stats"})
    assert list(got["ar"]["ar-stats"]) == list(ref["ar"]["ar-stats"])
    for k, v in ref["ar"]["ar-stats"].items():
        assert torch.equal(got["ar"]["ar-stats"][k], v) if torch.is_tensor(v) else got["ar"]["ar-stats"][k] == v, k
