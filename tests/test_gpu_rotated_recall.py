"""The slenderness-bucketed recall pass (AR / mAR) on rotated boxes on the MI355X (sod_proposal_ar_rotated, csrc/coco_eval_rotated.hip
over csrc/proposal_ar.h) against the restatement (tests/rotated_recall_restated.py).

The arbiter is the restatement handed HF.box_iou_rotated(dt, gt) of every image, copied to the host: the kernel behind it runs the
device function the recall kernel runs, so the same float32 bits go into both and hits, counts (integers) and recalls (one float32
division) are compared for exact equality - no tolerance is involved.  (The IoU values themselves are tested against the CPU oracle
in test_gpu_rotated_coco_eval.py.)"""
import json

import numpy as np
import pytest
import torch

import coco_eval_restated as RS
import rotated_recall_restated as AR
import test_rotated_recall_host as H
from test_coco_eval_host import _same, assert_results_equal, assert_ulp
from test_gpu_rotated_coco_eval import gpu_iou

from slenderobjdet_amd.data.catalog import MetadataCatalog
from slenderobjdet_amd.evaluation import RotatedCOCOEvaluator
from slenderobjdet_amd.evaluation import device as D
from slenderobjdet_amd.evaluation.coco_evaluation import predictions_from_numpy
from slenderobjdet_amd.evaluation.coco_gt import CocoGt
from slenderobjdet_amd.evaluation.rotated_coco_evaluation import boxes_to_rotated

pytestmark = pytest.mark.gpu

CATS3 = (2, 5, 9)       # dataset category ids -> contiguous 0, 1, 2


def _boxes(rs, n):
    """[n, 5]: sides 4 - 200 px, side ratio 1:1 .. 1:20 (log-uniform), either side the long one, angle in (-90, 90]."""
    q = np.exp(rs.uniform(0.0, np.log(20.0), n))
    long_ = rs.uniform(np.maximum(4.0 * q, 4.0), 200.0)
    short = long_ / q
    swap = rs.rand(n) < 0.5
    w, h = np.where(swap, short, long_), np.where(swap, long_, short)
    ang = 90.0 - rs.uniform(0.0, 180.0, n)
    return np.stack([rs.uniform(100, 540, n), rs.uniform(100, 380, n), w, h, ang], axis=1).astype(np.float32)


def _jitter(rs, b, s=1.0):
    """Detections around the boxes b: centre, sides and angle disturbed, sides kept within 4 - 200 px."""
    out = b + rs.randn(*b.shape).astype(np.float32) * np.array([3, 3, 4, 4, 5], np.float32) * np.float32(s)
    out[:, 2:4] = np.clip(out[:, 2:4], 4, 200)
    out[:, 4] = np.clip(out[:, 4], -89.5, 90)
    return out.astype(np.float32)


def _case(seed, shapes, cats=CATS3, wrong_class=0.2):
    """shapes: (G, D) per image.  Detections: jittered gts (class of the gt, or with probability ``wrong_class`` another one) in random
    order, the rest random boxes."""
    rs = np.random.RandomState(seed)
    images, anns, rows = [], [], []
    for i, (G, Dn) in enumerate(shapes):
        img = 40 - 3 * i                                  # descending ids: the sorted image order is not the json order
        images.append({"id": img, "width": 640, "height": 480})
        g = _boxes(rs, G)
        gc = rs.randint(0, len(cats), G)
        for b, c in zip(g, gc):
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cats[c], "bbox": [float(v) for v in b],
                         "area": float(b[2]) * float(b[3]), "iscrowd": 0})
        if G and Dn:
            pick = rs.randint(0, G, Dn)
            d = _jitter(rs, g[pick], s=rs.uniform(0.2, 2.0))
            dc = np.where(rs.rand(Dn) < wrong_class, rs.randint(0, len(cats), Dn), gc[pick])
            far = rs.rand(Dn) < 0.2
            d[far] = _boxes(rs, int(far.sum()))
        else:
            d, dc = _boxes(rs, Dn), rs.randint(0, len(cats), Dn)
        rows += [(img, int(c), b) for b, c in zip(d, dc)]
    order = rs.permutation(len(rows))                     # the images' predictions interleaved: prediction order is per image
    rows = [rows[j] for j in order]
    ds = {"images": images, "annotations": anns, "categories": [{"id": c, "name": f"c{c}"} for c in cats]}
    return ds, _preds(rows)


def _preds(rows):
    return {"image_id": np.array([r[0] for r in rows], np.int64), "category": np.array([r[1] for r in rows], np.int64),
            "boxes": np.array([r[2] for r in rows], np.float32).reshape(len(rows), 5),
            "score": np.linspace(0.99, 0.01, len(rows)).astype(np.float32)}


def _restated(ds, preds, iou_fn=gpu_iou):
    gt, by_img, _, images5 = H.restated_inputs(ds, preds)
    return gt, AR.proposal_ar_rotated(images5, by_img, gt.id_map, len(gt.cat_ids), iou_fn)


def _run(cuda, ds, preds):
    gt = CocoGt(ds)
    gd = D.RotatedGtDevice(gt, cuda)
    flat = predictions_from_numpy(preds, cuda)
    out = D.run_rotated_ar(gd, flat["image_id"], boxes_to_rotated(flat["boxes"]), flat["scores"], flat["classes"])
    return gd, {k: v.cpu() for k, v in out.items()}


def _check(cuda, ds, preds):
    """The kernel's hits, counts and recalls equal the restatement's on the device's own IoUs.  Returns (restated hits, num_pos, used)."""
    gd, out = _run(cuda, ds, preds)
    gt, (recalls, ar, mar, num_pos, used, hits) = _restated(ds, preds)
    K1 = len(gt.cat_ids) + 1
    assert out["hits"].dtype == torch.int32 and out["counts"].dtype == torch.int32 and out["recalls"].dtype == torch.float32
    assert tuple(out["hits"].shape) == (10, K1, 6, 4) == tuple(out["recalls"].shape) and tuple(out["counts"].shape) == (K1, 6, 4)
    _same(out["counts"].numpy().astype(np.int64), num_pos.numpy())
    _same(out["hits"].numpy().astype(np.int64), hits.numpy())
    _same(out["recalls"].numpy(), recalls.numpy())
    return gd, hits, num_pos, used


# ------------------------------------------------------------------------------------------------ 1. small shapes
@pytest.mark.parametrize("name,shapes,cats", [("one_by_one", [(1, 1), (1, 1)], CATS3), ("fewer_dets", [(7, 3), (5, 2), (9, 4)], CATS3),
                                              ("more_dets", [(3, 11), (2, 17), (4, 9), (1, 6)], CATS3),
                                              ("one_class", [(4, 6), (6, 3), (2, 2)], (4,))])
def test_small_shapes(cuda, name, shapes, cats):
    ds, preds = _case(11 + len(name), shapes, cats)
    _, hits, num_pos, used = _check(cuda, ds, preds)
    assert used == len(shapes) and int(num_pos[-1, 0, 0]) == sum(g for g, _ in shapes)
    # the rounds of an image: min(D, G), each recorded once in "all ratios, all areas" at the lowest threshold if it hits
    assert 0 < int(hits[0, -1, 0, 0]) <= sum(min(g, d) for g, d in shapes)


# ------------------------------------------------------------------------------------------------ 2. images that take no part
def test_images_without_detections_or_without_gts(cuda):
    shapes = [(4, 5), (6, 0), (0, 7), (3, 8)]
    ds, preds = _case(21, shapes)
    _, hits, num_pos, used = _check(cuda, ds, preds)
    assert used == 2 and int(num_pos[-1, 0, 0]) == 4 + 3          # the six gts of the image without detections add nothing


# ------------------------------------------------------------------------------------------------ 3. truncation
def test_first_hundred_detections_in_prediction_order(cuda):
    ds, preds = _case(31, [(3, 130), (2, 4)])
    big = ds["images"][0]["id"]
    sel = np.nonzero(preds["image_id"] == big)[0]
    assert len(sel) == 130
    # the last 30 of the image in prediction order are exact copies of its gts with the gts' classes: taking part, they would win
    g = [a for a in ds["annotations"] if a["image_id"] == big]
    for n, j in enumerate(sel[100:]):
        a = g[n % 3]
        preds["boxes"][j] = np.array(a["bbox"], np.float32)
        preds["category"][j] = CATS3.index(a["category_id"])
    # ... and the first 100 hold jittered boxes only
    _, hits, num_pos, _ = _check(cuda, ds, preds)
    assert int(hits[-1, -1, 0, 0]) < 3                             # at IoU 0.95 the exact copies would hit all three gts
    keep = np.setdiff1d(np.arange(len(preds["score"])), sel[100:])
    _, (_, _, _, _, _, hits_cut) = _restated(ds, {k: v[keep] for k, v in preds.items()})
    _same(hits.numpy(), hits_cut.numpy())


# ------------------------------------------------------------------------------------------------ 4. scratch path
@pytest.mark.parametrize("G,Dn", [(40, 100), (300, 12)])
def test_scratch_path_beside_an_lds_image(cuda, G, Dn):
    ds, preds = _case(41 + G, [(5, 9), (G, Dn), (3, 2)])
    assert G * min(Dn, 100) > 3200
    gd, hits, num_pos, used = _check(cuda, ds, preds)
    r = gd.recall()
    assert used == 3 and r["scratch"].numel() == 2 * 100 * G
    sizes = np.diff(np.concatenate([r["scratch_off"].cpu().numpy(), [r["scratch"].numel()]]))
    assert sorted(sizes.tolist()) == [0, 0, 2 * 100 * G]
    assert int(hits[0, -1, 0, 0]) > 5                              # the large image's rounds hit too


# ------------------------------------------------------------------------------------------------ 5. class-aware against class-agnostic
def test_class_aware_and_class_agnostic_winners_differ(cuda):
    rs = np.random.RandomState(51)
    images, anns, rows = [], [], []
    for i, G in enumerate((4, 6, 3)):
        img = 7 + i
        images.append({"id": img, "width": 640, "height": 480})
        g = _boxes(rs, G)
        g[:, 0] = 60 + 110 * np.arange(G)                          # apart from each other
        gc = rs.randint(0, 3, G)
        for b, c in zip(g, gc):
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": CATS3[c], "bbox": [float(v) for v in b],
                         "area": float(b[2]) * float(b[3]), "iscrowd": 0})
        tight, loose = _jitter(rs, g, 0.1), _jitter(rs, g, 0.8)
        # the tight detection carries another class, the loose one the gt's; one gt gets a tight detection only
        for n in range(G):
            rows.append((img, int((gc[n] + 1) % 3), tight[n]))
            if n:
                rows.append((img, int(gc[n]), loose[n]))
    ds = {"images": images, "annotations": anns, "categories": [{"id": c, "name": f"c{c}"} for c in CATS3]}
    _, hits, num_pos, _ = _check(cuda, ds, _preds(rows))
    agnostic, aware = hits[:, -1, 0, 0], hits[:, :-1, 0, 0].sum(dim=1)
    assert int(agnostic.sum()) > int(aware.sum()) > 0


# ------------------------------------------------------------------------------------------------ 6. ties
def test_duplicates_and_a_gt_with_a_zero_side(cuda):
    ds, preds = _case(61, [(4, 6), (5, 5)], wrong_class=0.0)
    rows = [(int(i), int(c), b) for i, c, b in zip(preds["image_id"], preds["category"], preds["boxes"])]
    img0, img1 = ds["images"][0]["id"], ds["images"][1]["id"]
    a0 = [a for a in ds["annotations"] if a["image_id"] == img0]
    # image 0: gt 2 is an exact duplicate of gt 0 (class included); three exact duplicate detections on it, of its class
    a0[2]["bbox"], a0[2]["category_id"], a0[2]["area"] = list(a0[0]["bbox"]), a0[0]["category_id"], a0[0]["area"]
    dup = (img0, CATS3.index(a0[0]["category_id"]), _jitter(np.random.RandomState(62), np.array([a0[0]["bbox"]], np.float32), 0.3)[0])
    rows = [dup] + rows[:5] + [dup] + rows[5:] + [dup]
    # image 1: a gt with a zero side (it overlaps nothing and sits in the ratio bucket "0 - 1/5" and the area bucket "small")
    a1 = [a for a in ds["annotations"] if a["image_id"] == img1]
    a1[1]["bbox"][2], a1[1]["area"] = 0.0, 0.0
    _, hits, num_pos, used = _check(cuda, ds, _preds(rows))
    assert used == 2 and int(num_pos[-1, 0, 0]) == 9 and int(num_pos[-1, 1, 1]) >= 1


# ------------------------------------------------------------------------------------------------ 7. angle 0
def test_angle0_equals_the_axis_aligned_kernel(cuda):
    ds, preds = H.angle0_fixture()
    gt, by_img, _, images5 = H.restated_inputs(ds, preds)
    H.assert_fixture_condition(by_img, images5, gt.id_map)
    _, out = _run(cuda, ds, preds)                                 # four-column XYXY predictions through boxes_to_rotated
    flat = predictions_from_numpy(preds, cuda)
    ref = D.run(D.GtDevice(CocoGt(ds), cuda), flat["image_id"], flat["boxes"], flat["scores"], flat["classes"])
    assert torch.equal(out["counts"], ref["counts"].cpu()) and int(out["counts"][-1, 0, 0]) == 8
    assert torch.equal(out["hits"], ref["hits"].cpu()) and int(out["hits"][0, -1, 0, 0]) == 7
    assert torch.equal(out["recalls"], ref["recalls"].cpu())


# ------------------------------------------------------------------------------------------------ 8. through the evaluator
def _evaluator(tmp_path, name, dataset, recall, **kw):
    jf = tmp_path / f"{name}.json"
    jf.write_text(json.dumps(dataset))
    gt = CocoGt(dataset)
    meta = MetadataCatalog.get(name)
    meta.clear()
    meta.update(name=name, json_file=str(jf), thing_dataset_id_to_contiguous_id=dict(gt.id_map),
                thing_classes=[gt.cats[c]["name"] for c in gt.cat_ids])
    if recall:
        meta.rotated_recall = True
    return RotatedCOCOEvaluator(name, None, False, **kw)


def test_through_the_evaluator(cuda, tmp_path):
    ds, preds = _case(81, [(5, 12), (8, 6), (0, 4), (3, 0), (6, 20)])
    flat = predictions_from_numpy(preds, cuda)
    plain = _evaluator(tmp_path, "rot_recall_off", ds, False)
    res0 = plain.evaluate_flat(flat)
    assert list(res0) == ["bbox"] and plain.recalls is None and plain._gt_dev._recall is None      # nothing uploaded, nothing laid out
    ev = _evaluator(tmp_path, "rot_recall_on", ds, True)
    res = ev.evaluate_flat(flat)
    assert list(res) == ["bbox", "ar"]
    assert_results_equal(res["bbox"], res0["bbox"])
    _same(ev.precision, plain.precision)
    gt, (recalls, ar, mar, num_pos, _, _) = _restated(ds, preds)
    _same(ev.recalls.numpy(), recalls.numpy())
    st = res["ar"]["ar-stats"]
    _same(st["num_pos"].numpy(), num_pos.numpy())
    assert_ulp(st["ar"].numpy(), ar.numpy())
    assert_ulp(st["mar"].numpy(), mar.numpy())
    assert_results_equal({k: v for k, v in res["ar"].items() if k != "ar-stats"}, RS.ar_results(recalls, ar, mar, num_pos))
    assert res["ar"]["AR@100"] > 0
    # beside the ratio-bucketed AP the recall pass comes last
    both = _evaluator(tmp_path, "rot_recall_both", ds, True, ratio_buckets=True)
    res2 = both.evaluate_flat(flat)
    assert list(res2) == ["bbox", "bbox-ratios", "ar"]
    assert_results_equal({k: v for k, v in res2["ar"].items() if k != "ar-stats"}, {k: v for k, v in res["ar"].items() if k != "ar-stats"})


def test_empty_predictions_through_the_evaluator(cuda, tmp_path):
    ds, preds = _case(82, [(5, 3), (2, 2)])
    ev = _evaluator(tmp_path, "rot_recall_empty", ds, True)
    res = ev.evaluate_flat(predictions_from_numpy({k: v[:0] for k, v in preds.items()}, cuda))
    assert list(res) == ["bbox", "ar"]
    assert ev.recalls.shape == (10, 4, 6, 4) and bool((ev.recalls == 0).all())
    assert all(v == 0.0 for k, v in res["ar"].items() if k != "ar-stats")
    assert int(res["ar"]["ar-stats"]["num_pos"].sum()) == 0       # no image took part
    # evaluate() with processed images but no instances at all takes the same path
    ev.reset()
    ev.process([{"image_id": ds["images"][0]["id"]}], [{}])
    res = ev.evaluate()
    assert list(res) == ["bbox", "ar"] and res["ar"]["AR@100"] == 0.0
