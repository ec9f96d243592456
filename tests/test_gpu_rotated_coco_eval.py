"""Rotated-box COCO evaluation on the MI355X (csrc/coco_eval_rotated.hip + sod_coco_accumulate) against the restatement
(tests/rotated_coco_eval_restated.py).

The decision logic and the IoU values are tested separately, as test_nms_rotated_keep_indices does: with ~10^5 pairs some IoU always
sits within float noise of a threshold, so the matching is compared bit for bit on shared IoUs - the restated matcher is handed
HF.box_iou_rotated(dt, gt) of every segment, the kernel behind which runs the same device function as the evaluator's kernel - and
the IoU values are compared with the CPU oracle on a small case (through HF.box_iou_rotated, not through a debug output of the
evaluator), together with that case's whole evaluation against the pure-CPU restatement."""
import json
import math

import numpy as np
import pytest
import torch

import rotated_coco_eval_restated as RR
import test_rotated_coco_eval_host as H
from test_coco_eval_host import _same, assert_results_equal

from slenderobjdet_amd.data.catalog import MetadataCatalog
from slenderobjdet_amd.evaluation import RotatedCOCOEvaluator, inference_on_dataset
from slenderobjdet_amd.evaluation.coco_evaluation import predictions_from_numpy
from slenderobjdet_amd.evaluation.coco_gt import CocoGt
from slenderobjdet_amd.evaluation.synthetic import synthetic_rotated_coco

pytestmark = pytest.mark.gpu


def _evaluator(tmp_path, name, dataset, with_names=True, **kw):
    jf = tmp_path / f"{name}.json"
    jf.write_text(json.dumps(dataset))
    gt = CocoGt(dataset)
    meta = MetadataCatalog.get(name)
    meta.clear()
    meta.update(name=name, json_file=str(jf), thing_dataset_id_to_contiguous_id=dict(gt.id_map))
    if with_names:
        meta["thing_classes"] = [gt.cats[c]["name"] for c in gt.cat_ids]
    return RotatedCOCOEvaluator(name, None, False, **kw)


def gpu_iou(dt, gt):
    from slenderobjdet_amd.layers import functional as HF

    d = torch.from_numpy(np.ascontiguousarray(dt, np.float32)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(gt, np.float32)).cuda()
    return HF.box_iou_rotated(d, g).cpu().numpy()


def _names(ds):
    return [c["name"] for c in sorted(ds["categories"], key=lambda c: c["id"])]


def _check_against_restatement(ev, ds, preds, res, iou_fn=gpu_iou, ratio=False):
    precision, recall, scores = H.restated_eval(ds, preds, "area", iou_fn)
    _same(ev.precision, precision)
    _same(ev.recall, recall)
    _same(ev.scores, scores)
    n = len(preds["score"])
    stats = RR.summarize_area(precision, recall) if n else None
    if n:
        _same(ev.stats, stats)
    else:
        assert ev.stats is None
    assert_results_equal(res["bbox"], RR.derive_results(stats, precision, _names(ds)))
    if ratio:
        precision, recall, _ = H.restated_eval(ds, preds, "ratio", iou_fn)
        _same(ev.ratio_precision, precision)
        _same(ev.ratio_recall, recall)
        stats = RR.RS.summarize(precision, recall) if n else None
        if n:
            _same(ev.ratio_stats, stats)
        assert list(res) == ["bbox", "bbox-ratios"]
        assert_results_equal(res["bbox-ratios"], RR.derive_ratio_results(stats))
    else:
        assert list(res) == ["bbox"]
    return stats


@pytest.mark.parametrize("seed", [201, 202, 203])
def test_matching_bit_exact_on_shared_ious(cuda, tmp_path, seed):
    ds, preds = synthetic_rotated_coco(seed, n_images=300, n_cats=30, dets_per_image=(0, 40), score_levels=50 if seed == 203 else None,
                                       dup=0.05 if seed == 203 else 0.0)
    ev = _evaluator(tmp_path, f"rot_random_{seed}", ds)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    stats = _check_against_restatement(ev, ds, preds, res)
    assert 0.0 < stats[0] < 1.0 and stats[8] > 0.1          # a real mixture of hits and misses


SMALL_SEED = 3      # chosen on the CPU: 160 pairs, the oracle's closest IoU 3.3e-3 away from a threshold


def test_iou_values_and_small_case_against_cpu_oracle(cuda, tmp_path):
    ds, preds = synthetic_rotated_coco(SMALL_SEED, n_images=8, n_cats=2, dets_per_image=(2, 8))
    img_ids, cat_ids, gts, dets = RR.restated_inputs(ds, preds)
    pairs, worst, near = 0, 0.0, 1.0
    for img in img_ids:
        for c in cat_ids:
            g = [x["box5"] for x in gts if x["image_id"] == img and x["category_id"] == c]
            dn = np.nonzero((dets["image_id"] == img) & (dets["category_id"] == c))[0]
            if not g or not len(dn):
                continue
            ref = RR.oracle_iou(dets["box5"][dn], np.stack(g))
            got = gpu_iou(dets["box5"][dn], np.stack(g))
            pairs += ref.size
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
            near = min(near, float(np.abs(ref.astype(np.float64)[..., None] - RR.IOU_THRS).min()))
    print(f"pairs {pairs}  max |gpu - oracle| {worst:.3e}  oracle's closest distance to a threshold {near:.3e}")
    assert 100 <= pairs <= 400 and near >= 2e-4
    assert worst < 2e-4
    ev = _evaluator(tmp_path, "rot_small", ds, ratio_buckets=True)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    _check_against_restatement(ev, ds, preds, res, iou_fn=RR.oracle_iou, ratio=True)      # the whole evaluation, pure CPU reference


def test_hand_derived_cases_through_the_kernels(cuda, tmp_path):
    out = []
    for swapped in (False, True):
        ds, preds = H.case_perfect(swapped)
        ev = _evaluator(tmp_path, f"rot_perfect_{int(swapped)}", ds)
        res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
        H.check_perfect(ev.stats, res["bbox"])
        _check_against_restatement(ev, ds, preds, res)
        out.append((ev.precision, ev.recall, ev.scores, ev.stats))
    for a, b in zip(*out):
        _same(a, b)
    ds, preds = H.case_squares()
    ev = _evaluator(tmp_path, "rot_squares", ds)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    H.check_squares(ev.recall, ev.stats, res["bbox"])
    ds, preds = H.case_area_buckets()
    ev = _evaluator(tmp_path, "rot_areas", ds)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    H.check_area_buckets(ev.stats, res["bbox"])
    _check_against_restatement(ev, ds, preds, res)


def _crowded_case(seed):
    """One image whose single category holds > 64 gts and > 100 detections: the global scratch slot for the IoUs and the bit rows."""
    ds, preds = synthetic_rotated_coco(seed, n_images=6, n_cats=2, dets_per_image=(5, 20))
    rs = np.random.RandomState(seed)
    img = ds["images"][0]["id"]
    cat = sorted(c["id"] for c in ds["categories"])[0]
    nid = max(a["id"] for a in ds["annotations"]) + 1
    boxes = []
    for j in range(90):
        b = [float(rs.randint(0, 600)), float(rs.randint(0, 440)), float(rs.randint(8, 40)), float(rs.randint(8, 40)), float(rs.randint(-89, 91))]
        ds["annotations"].append({"id": nid + j, "image_id": img, "category_id": cat, "bbox": b, "area": b[2] * b[3], "iscrowd": 0})
        boxes.append(b)
    boxes = np.array(boxes, np.float32)
    pick = rs.randint(0, len(boxes), 130)
    jit = (boxes[pick] + rs.randn(130, 5).astype(np.float32) * np.array([2, 2, 2, 2, 3], np.float32)).astype(np.float32)
    jit[:, 2:4] = np.maximum(jit[:, 2:4], 1)
    preds["image_id"] = np.concatenate([preds["image_id"], np.full(130, img, np.int64)])
    preds["category"] = np.concatenate([preds["category"], np.zeros(130, np.int64)])
    preds["boxes"] = np.concatenate([preds["boxes"], jit])
    preds["score"] = np.concatenate([preds["score"], rs.rand(130).astype(np.float32)])
    return ds, preds


def test_scratch_paths(cuda, tmp_path):
    ds, preds = _crowded_case(7)
    # a second crowded segment with <= 64 gts whose IoU matrix alone outgrows the LDS (40 gts x 100 detections)
    rs = np.random.RandomState(70)
    img = ds["images"][1]["id"]
    cat = sorted(c["id"] for c in ds["categories"])[1]
    nid = max(a["id"] for a in ds["annotations"]) + 1
    extra = []
    for j in range(40):
        b = [float(rs.randint(0, 600)), float(rs.randint(0, 440)), float(rs.randint(8, 60)), float(rs.randint(8, 60)), float(rs.randint(-89, 91))]
        ds["annotations"].append({"id": nid + j, "image_id": img, "category_id": cat, "bbox": b, "area": b[2] * b[3], "iscrowd": 0})
        extra.append(b)
    extra = np.array(extra, np.float32)[rs.randint(0, 40, 110)] + rs.randn(110, 5).astype(np.float32)
    extra[:, 2:4] = np.maximum(extra[:, 2:4], 1)
    preds["image_id"] = np.concatenate([preds["image_id"], np.full(110, img, np.int64)])
    preds["category"] = np.concatenate([preds["category"], np.ones(110, np.int64)])
    preds["boxes"] = np.concatenate([preds["boxes"], extra.astype(np.float32)])
    preds["score"] = np.concatenate([preds["score"], rs.rand(110).astype(np.float32)])
    ev = _evaluator(tmp_path, "rot_crowded", ds, ratio_buckets=True)
    counts = np.diff(ev._gt.rotated_arrays()["seg_gt_off"])
    assert counts.max() > 64 and ((counts > 32) & (counts <= 64)).any()
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    assert ev._gt_dev.match_scratch.numel() > 2
    _check_against_restatement(ev, ds, preds, res, ratio=True)


def test_empty_predictions(cuda, tmp_path):
    ds, preds = synthetic_rotated_coco(8, n_images=10, n_cats=3)
    preds = {k: v[:0] for k, v in preds.items()}
    ev = _evaluator(tmp_path, "rot_empty", ds, ratio_buckets=True)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    assert list(res["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    assert all(math.isnan(v) for v in res["bbox"].values()) and all(math.isnan(v) for v in res["bbox-ratios"].values())
    _check_against_restatement(ev, ds, preds, res, ratio=True)
    # evaluate() with processed images but no instances at all takes the same path
    ev.reset()
    ev.process([{"image_id": ds["images"][0]["id"]}], [{}])
    res = ev.evaluate()
    assert list(res) == ["bbox", "bbox-ratios"] and all(math.isnan(v) for v in res["bbox"].values())


def test_images_and_categories_without_gts(cuda, tmp_path):
    ds, preds = synthetic_rotated_coco(12, n_images=40, n_cats=5, dets_per_image=(3, 15), no_gt=0.4)
    cats = sorted(c["id"] for c in ds["categories"])
    ds["annotations"] = [a for a in ds["annotations"] if a["category_id"] != cats[2]]          # a category without any gt
    assert sum(1 for im in ds["images"] if not any(a["image_id"] == im["id"] for a in ds["annotations"])) >= 5
    assert (preds["category"] == 2).any()
    ev = _evaluator(tmp_path, "rot_nogt", ds)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    _check_against_restatement(ev, ds, preds, res)
    assert math.isnan(res["bbox"]["AP-" + _names(ds)[2]]) and np.all(ev.precision[:, :, 2] == -1)


def test_four_column_predictions_and_xywh_gts(cuda, tmp_path):
    from slenderobjdet_amd.evaluation.synthetic import synthetic_coco

    ds, preds = synthetic_coco(13, n_images=30, n_cats=4, dets_per_image=(2, 15), crowd=0.05)
    assert preds["boxes"].shape[1] == 4 and any(a["iscrowd"] for a in ds["annotations"])      # crowd gts are fine without rotated gts
    ev = _evaluator(tmp_path, "rot_xyxy", ds, ratio_buckets=True)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    _check_against_restatement(ev, ds, preds, res, ratio=True)
    # the same predictions handed over in centre form give the same arrays
    p5 = dict(preds, boxes=RR.pred_box5(preds["boxes"]))
    precision = ev.precision
    ev.evaluate_flat(predictions_from_numpy(p5, cuda))
    _same(ev.precision, precision)


def test_default_output_and_results_json(cuda, tmp_path):
    from slenderobjdet_amd.structures import Instances, RotatedBoxes

    ds, preds = synthetic_rotated_coco(14, n_images=12, n_cats=3, dets_per_image=(1, 9))
    out_dir = tmp_path / "out"
    ev = _evaluator(tmp_path, "rot_json", ds, output_dir=str(out_dir))
    inputs, outputs = [], []
    for img in [im["id"] for im in ds["images"]]:
        sel = np.nonzero(preds["image_id"] == img)[0]
        inst = Instances((480, 640))
        inst.pred_boxes = RotatedBoxes(torch.from_numpy(preds["boxes"][sel]).to(cuda))
        inst.scores = torch.from_numpy(preds["score"][sel]).to(cuda)
        inst.pred_classes = torch.from_numpy(preds["category"][sel]).to(cuda)
        inputs.append({"image_id": img})
        outputs.append({"instances": inst})
    ev.process(inputs, outputs)
    res = ev.evaluate()
    assert list(res) == ["bbox"]
    assert list(res["bbox"])[:6] == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and len(res["bbox"]) == 9
    rows = json.loads((out_dir / "coco_instances_results.json").read_text())
    assert len(rows) == len(preds["score"]) and all(len(r["bbox"]) == 5 for r in rows)
    cats = sorted(c["id"] for c in ds["categories"])
    # the written file, read back as predictions, evaluates to the same numbers
    back = {"image_id": np.array([r["image_id"] for r in rows], np.int64),
            "category": np.array([cats.index(r["category_id"]) for r in rows], np.int64),
            "boxes": np.array([r["bbox"] for r in rows], np.float32), "score": np.array([r["score"] for r in rows], np.float32)}
    _check_against_restatement(ev, ds, back, res)


def test_process_does_not_synchronise(cuda, tmp_path, monkeypatch):
    """Twin of test_gpu_coco_eval.py::test_process_does_not_synchronise for the rotated evaluator."""
    from slenderobjdet_amd.structures import Instances, RotatedBoxes

    ds, preds = synthetic_rotated_coco(10, n_images=8, n_cats=3)
    ev = _evaluator(tmp_path, "rot_nosync", ds)
    inputs, outputs = [], []
    for img in [im["id"] for im in ds["images"]]:
        sel = np.nonzero(preds["image_id"] == img)[0]
        inst = Instances((480, 640))
        inst.pred_boxes = RotatedBoxes(torch.from_numpy(preds["boxes"][sel]).to(cuda))
        inst.scores = torch.from_numpy(preds["score"][sel]).to(cuda)
        inst.pred_classes = torch.from_numpy(preds["category"][sel]).to(cuda)
        inputs.append({"image_id": img})
        outputs.append({"instances": inst})
    torch.cuda.synchronize()
    probe = torch.ones(1, device=cuda)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            sync_mode_works = False
        except RuntimeError:
            sync_mode_works = True
        if sync_mode_works:
            ev.process(inputs, outputs)
    finally:
        torch.cuda.set_sync_debug_mode(0)

    def _fail(*a, **k):
        raise AssertionError("process() synchronised with the device")

    ev.reset()
    with monkeypatch.context() as m:
        for name in ("item", "tolist", "cpu", "numpy", "__bool__", "__int__", "__float__", "nonzero"):
            m.setattr(torch.Tensor, name, _fail)
        m.setattr(torch.cuda, "synchronize", _fail)
        ev.process(inputs, outputs)
    assert len(ev._chunks) == len(inputs) and all(c[1].is_cuda and c[0].is_cuda for c in ev._chunks)
    res = ev.evaluate_flat(ev._flat())
    _check_against_restatement(ev, ds, preds, res)


def _rotated_json_for_batches(batches):
    images, anns, aid = [], [], 1
    for batch in batches:
        for d in batch:
            images.append({"id": d["image_id"], "width": d["width"], "height": d["height"]})
            inst = d["instances"]
            for box, c in zip(inst.gt_boxes.tensor.cpu().tolist(), inst.gt_classes.cpu().tolist()):
                anns.append({"id": aid, "image_id": d["image_id"], "category_id": int(c) + 1, "bbox": box, "area": box[2] * box[3], "iscrowd": 0})
                aid += 1
    return {"images": images, "annotations": anns, "categories": [{"id": c + 1, "name": f"c{c}"} for c in range(80)]}


def test_end_to_end_rotated_rcnn_inference_on_dataset(cuda, tmp_path):
    """configs/rotated/Base-RRCNN-FPN.yaml at a small size with random weights, through inference_on_dataset."""
    from test_gpu_rcnn import _cfg, _data

    from slenderobjdet_amd.modeling import build_model

    cfg = _cfg(rotated=True)
    torch.manual_seed(5)
    model = build_model(cfg)
    model.roi_heads.box_predictor.test_score_thresh = 0.0      # random weights: every class sits near 1 / 81
    loader = []
    for b in range(3):
        batch = _data(2, 96, 128, 400 + b, True)
        for j, d in enumerate(batch):
            d["image_id"] = 2000 + 2 * b + j
            d.setdefault("height", 96)
            d.setdefault("width", 128)
        loader.append(batch)
    ds = _rotated_json_for_batches(loader)
    # distinct gt boxes per (image, category), so that each fed-back gt matches itself best
    seen = set()
    for a in ds["annotations"]:
        key = (a["image_id"], a["category_id"], tuple(a["bbox"]))
        assert key not in seen
        seen.add(key)
    ev = _evaluator(tmp_path, "rot_e2e", ds, ratio_buckets=True)
    res = inference_on_dataset("rot_e2e", model, loader, ev)
    assert list(res) == ["bbox", "bbox-ratios"]
    assert list(res["bbox"])[:6] == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and len(res["bbox"]) == 6 + 80
    assert all(math.isnan(v) or (0.0 <= v <= 100.0) for v in res["bbox"].values())
    assert all(math.isnan(v) or (0.0 <= v <= 100.0) for v in res["bbox-ratios"].values())
    flat = ev._flat()
    assert flat is not None and flat["scores"].shape[0] > 0 and flat["boxes"].shape[1] == 5
    preds = {"image_id": flat["image_id"].cpu().numpy(), "category": flat["classes"].cpu().numpy(),
             "boxes": flat["boxes"].cpu().numpy().astype(np.float32), "score": flat["scores"].cpu().numpy().astype(np.float32)}
    _check_against_restatement(ev, ds, preds, res, ratio=True)
    # the gts fed back as predictions with score 1: AP = 100
    back = {"image_id": np.array([a["image_id"] for a in ds["annotations"]], np.int64),
            "category": np.array([a["category_id"] - 1 for a in ds["annotations"]], np.int64),
            "boxes": np.array([a["bbox"] for a in ds["annotations"]], np.float32), "score": np.ones(len(ds["annotations"]), np.float32)}
    res = ev.evaluate_flat(predictions_from_numpy(back, cuda))
    assert H._eq(res["bbox"]["AP"], 100.0) and H._eq(res["bbox"]["AP50"], 100.0) and H._eq(res["bbox"]["AP75"], 100.0)
    assert ev.stats[8] == 1.0
