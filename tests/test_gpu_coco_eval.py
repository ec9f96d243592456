"""Slender-object COCO evaluation on the MI355X: the three HIP passes (csrc/coco_eval.hip) against the reference's fixtures and
against the restatement (tests/coco_eval_restated.py), bit for bit; the perfect predictor; the end-to-end FCOS path through
inference_on_dataset; and a process() that never waits for the device."""
import json
import math

import numpy as np
import pytest
import torch

import coco_eval_restated as RS
from test_coco_eval_host import CASES, _same, assert_results_equal, assert_ulp, load_case, restated_inputs

from slenderobjdet_amd.data.catalog import MetadataCatalog
from slenderobjdet_amd.evaluation import COCOEvaluator, inference_on_dataset
from slenderobjdet_amd.evaluation.coco_evaluation import predictions_from_numpy
from slenderobjdet_amd.evaluation.coco_gt import CocoGt
from slenderobjdet_amd.evaluation.synthetic import synthetic_coco

pytestmark = pytest.mark.gpu


def _evaluator(tmp_path, name, dataset, with_names=True):
    jf = tmp_path / f"{name}.json"
    jf.write_text(json.dumps(dataset))
    gt = CocoGt(dataset)
    meta = MetadataCatalog.get(name)
    meta.clear()
    meta.update(name=name, json_file=str(jf), thing_dataset_id_to_contiguous_id=dict(gt.id_map))
    if with_names:
        meta["thing_classes"] = [gt.cats[c]["name"] for c in gt.cat_ids]
    return COCOEvaluator(name, None, False)


def _check_against_restatement(ev, dataset, preds, res):
    d = {"dataset": dataset, "pred_image_id": preds["image_id"], "pred_category": preds["category"], "pred_boxes": preds["boxes"],
         "pred_score": preds["score"], "pred_order": np.array([im["id"] for im in dataset["images"]], np.int64)}
    gt, gts, dets, by_img, images = restated_inputs(d)
    precision, recall, scores = RS.match_and_accumulate(gt.img_ids, gt.cat_ids, gts, dets)
    _same(ev.precision, precision)
    _same(ev.recall, recall)
    _same(ev.scores, scores)
    if len(preds["score"]):
        stats = RS.summarize(precision, recall)
        _same(ev.stats, stats)
        assert_results_equal(res["bbox"], RS.derive_bbox_results(stats, precision, [gt.cats[c]["name"] for c in gt.cat_ids]))
    recalls, ar, mar, num_pos, _ = RS.proposal_ar(images, by_img, gt.id_map, len(gt.cat_ids))
    _same(ev.recalls.numpy(), recalls.numpy())
    _same(res["ar"]["ar-stats"]["num_pos"].numpy(), num_pos.numpy())
    assert_ulp(res["ar"]["ar-stats"]["ar"].numpy(), ar.numpy())
    assert_ulp(res["ar"]["ar-stats"]["mar"].numpy(), mar.numpy())
    got = {k: v for k, v in res["ar"].items() if k != "ar-stats"}
    assert_results_equal(got, RS.ar_results(recalls, ar, mar, num_pos))


@pytest.mark.parametrize("case", CASES)
def test_kernels_match_reference_fixture(cuda, tmp_path, case):
    d = load_case(case)
    ev = _evaluator(tmp_path, f"fixture_{case}", d["dataset"])
    preds = {"image_id": d["pred_image_id"], "boxes": d["pred_boxes"], "score": d["pred_score"], "category": d["pred_category"]}
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    _same(ev.precision, d["precision"])
    _same(ev.recall, d["recall"])
    _same(ev.scores, d["scores"])
    _same(ev.stats, d["stats"])
    assert list(res) == ["ar", "bbox"]
    assert_results_equal(res["bbox"], d["bbox_results"])
    _same(ev.recalls.numpy(), d["ar_recalls"])
    st = res["ar"]["ar-stats"]
    _same(st["num_pos"].numpy(), d["ar_num_pos"])
    assert_ulp(st["ar"].numpy(), d["ar_ar"])
    assert_ulp(st["mar"].numpy(), d["ar_mar"])
    assert_results_equal({k: v for k, v in res["ar"].items() if k != "ar-stats"}, d["ar_results"])


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_kernels_match_restatement_random(cuda, tmp_path, seed):
    ds, preds = synthetic_coco(seed, n_images=500, n_cats=80, dets_per_image=(0, 40), score_levels=50 if seed == 103 else None,
                               dup=0.05 if seed == 103 else 0.0)
    ev = _evaluator(tmp_path, f"random_{seed}", ds)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    _check_against_restatement(ev, ds, preds, res)


def _crowded_case(seed):
    """One image whose single category holds > 64 gts and > 100 detections: the global scratch paths of both passes."""
    ds, preds = synthetic_coco(seed, n_images=6, n_cats=2, dets_per_image=(5, 20))
    rs = np.random.RandomState(seed)
    img = ds["images"][0]["id"]
    cat = sorted(c["id"] for c in ds["categories"])[0]
    nid = max(a["id"] for a in ds["annotations"]) + 1
    boxes = []
    for j in range(90):
        x, y, w, h = float(rs.randint(0, 600)), float(rs.randint(0, 440)), float(rs.randint(8, 40)), float(rs.randint(8, 40))
        ds["annotations"].append({"id": nid + j, "image_id": img, "category_id": cat, "bbox": [x, y, w, h], "area": w * h,
                                  "iscrowd": int(j % 17 == 0)})
        boxes.append([x, y, x + w, y + h])
    boxes = np.array(boxes, np.float32)
    pick = rs.randint(0, len(boxes), 130)
    jit = (boxes[pick] + rs.randn(130, 4).astype(np.float32) * 2).astype(np.float32)
    jit[:, 2:] = np.maximum(jit[:, 2:], jit[:, :2] + 1)
    preds["image_id"] = np.concatenate([preds["image_id"], np.full(130, img, np.int64)])
    preds["category"] = np.concatenate([preds["category"], np.zeros(130, np.int64)])
    preds["boxes"] = np.concatenate([preds["boxes"], jit])
    preds["score"] = np.concatenate([preds["score"], rs.rand(130).astype(np.float32)])
    return ds, preds


def test_kernels_scratch_paths(cuda, tmp_path):
    ds, preds = _crowded_case(7)
    ev = _evaluator(tmp_path, "crowded", ds)
    assert np.diff(ev._gt.arrays()["seg_gt_off"]).max() > 64 and np.diff(ev._gt.arrays()["img_gt_off"]).max() > 64
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    assert ev._gt_dev.match_scratch.numel() > 1 and ev._gt_dev.ar_scratch.numel() > 1
    _check_against_restatement(ev, ds, preds, res)


def test_empty_predictions(cuda, tmp_path):
    ds, preds = synthetic_coco(8, n_images=10, n_cats=3)
    preds = {k: v[:0] for k, v in preds.items()}
    ev = _evaluator(tmp_path, "empty", ds)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    assert all(math.isnan(v) for v in res["bbox"].values())
    _check_against_restatement(ev, ds, preds, res)


def test_perfect_predictor(cuda, tmp_path):
    ds, _ = synthetic_coco(9, n_images=60, n_cats=5, crowd=0.0)
    gt = CocoGt(ds)
    b = np.array([a["bbox"] for a in ds["annotations"]], np.float32)
    preds = {"image_id": np.array([a["image_id"] for a in ds["annotations"]], np.int64),
             "category": np.array([gt.id_map[a["category_id"]] for a in ds["annotations"]], np.int64),
             "boxes": np.concatenate([b[:, :2], b[:, :2] + b[:, 2:]], axis=1), "score": np.ones(len(b), np.float32)}
    ev = _evaluator(tmp_path, "perfect", ds)
    res = ev.evaluate_flat(predictions_from_numpy(preds, cuda))
    bbox, ar = res["bbox"], res["ar"]
    has = [bool(((gt.ratios >= lo) & (gt.ratios <= hi)).any()) for lo, hi in RS.RATIO_RNG]
    assert bbox["AP"] == bbox["AP50"] == bbox["AP75"] == 100.0
    for key, h in zip(["APs", "APm", "APl"], has[1:4]):
        assert bbox[key] == 100.0 if h else math.isnan(bbox[key])
    assert not has[4] and not has[5] and ev.stats[6] == ev.stats[7] == -1 and ev.stats[14] == ev.stats[15] == -1
    assert np.allclose(ev.stats[[0, 1, 2, 10]], 1.0) and ev.stats[8] <= 1.0
    assert ar["AR@100"] == 100.0 and ar["AR-all areas@100"] == 100.0
    assert ar["AR-3/1 - 5/1@100"] == 0.0 and ar["AR-5/1 - INF@100"] == 0.0     # no gt there: 0 / max(0, 1)
    _check_against_restatement(ev, ds, preds, res)


def _coco_json_for_batches(batches):
    images, anns, aid = [], [], 1
    for batch in batches:
        for d in batch:
            images.append({"id": d["image_id"], "width": d["width"], "height": d["height"]})
            inst = d["instances"]
            for box, c in zip(inst.gt_boxes.tensor.cpu().tolist(), inst.gt_classes.cpu().tolist()):
                x1, y1, x2, y2 = box
                anns.append({"id": aid, "image_id": d["image_id"], "category_id": int(c) + 1, "bbox": [x1, y1, x2 - x1, y2 - y1],
                             "area": (x2 - x1) * (y2 - y1), "iscrowd": 0})
                aid += 1
    return {"images": images, "annotations": anns, "categories": [{"id": c + 1, "name": f"c{c}"} for c in range(80)]}


def test_end_to_end_fcos_inference_on_dataset(cuda, tmp_path):
    from bench import make_cfg
    from slenderobjdet_amd.data import synthetic_batch
    from slenderobjdet_amd.modeling import build_model

    cfg = make_cfg(depth=18)
    torch.manual_seed(4)
    model = build_model(cfg)
    with torch.no_grad():
        model.head.cls_pred.bias[:80] = -2.0
        model.head.cls_pred.weight[:80] *= 20
    model.arena.bump()
    loader = []
    for b in range(3):
        batch = synthetic_batch(2, 256, 320, 300 + b, device="cuda")
        for j, d in enumerate(batch):
            d["image_id"] = 1000 + 2 * b + j
        loader.append(batch)
    ds = _coco_json_for_batches(loader)
    ev = _evaluator(tmp_path, "e2e_synthetic", ds)
    res = inference_on_dataset("e2e_synthetic", model, loader, ev)
    assert list(res) == ["ar", "bbox"]
    flat = ev._flat()
    assert flat is not None and flat["scores"].shape[0] > 0
    preds = {"image_id": flat["image_id"].cpu().numpy(), "category": flat["classes"].cpu().numpy(),
             "boxes": flat["boxes"].cpu().numpy().astype(np.float32), "score": flat["scores"].cpu().numpy().astype(np.float32)}
    _check_against_restatement(ev, ds, preds, res)


def test_process_does_not_synchronise(cuda, tmp_path, monkeypatch):
    """process() keeps everything on the device.  torch.cuda.set_sync_debug_mode("error") is used where it trips on a deliberate
    .item() on this runtime; the host-side guard below (every tensor -> host path and device synchronise raise) holds in any case."""
    from slenderobjdet_amd.structures import Boxes, Instances

    ds, preds = synthetic_coco(10, n_images=8, n_cats=3)
    ev = _evaluator(tmp_path, "nosync", ds)
    inputs, outputs = [], []
    for img in [im["id"] for im in ds["images"]]:
        sel = np.nonzero(preds["image_id"] == img)[0]
        inst = Instances((480, 640))
        inst.pred_boxes = Boxes(torch.from_numpy(preds["boxes"][sel]).to(cuda))
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
