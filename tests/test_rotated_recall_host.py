"""The slenderness-bucketed recall pass (AR / mAR) on rotated boxes, host side (CPU): the gt arrays of
CocoGt.rotated_recall_arrays(), the C ABI's declaration and scratch-size query, the restatement (tests/rotated_recall_restated.py)
against the axis-aligned restatement on angle-0 boxes, and the result dict."""
import ctypes

import numpy as np
import pytest
import torch

import coco_eval_restated as RS
import rotated_coco_eval_restated as RR
import rotated_iou_loss_restated as RL
import rotated_recall_restated as AR
from test_coco_eval_host import _same
from test_rotated_coco_eval_host import _four_ann_dataset

from slenderobjdet_amd.evaluation.coco_gt import CocoGt
from slenderobjdet_amd.evaluation.results import ar_results


# ------------------------------------------------------------------------------------------------ gt arrays
def test_rotated_recall_arrays():
    ds = _four_ann_dataset()
    gt = CocoGt(ds)
    h = gt.rotated_recall_arrays()
    assert list(h) == ["img_gt_off", "img_box5", "img_cls", "img_ratio5"]
    assert [h[k].dtype for k in h] == [np.int32, np.float32, np.int32, np.float32]
    # img_ids [2, 9]: image 2 holds anns 2 and 4, image 9 anns 1 and 3, each in json order; id_map {3: 0, 7: 1}
    assert h["img_gt_off"].tolist() == [0, 2, 4] and h["img_box5"].shape == (4, 5)
    f = np.float32
    xywh = np.array([10.1, 20.2, 4.4, 8.6], f)
    want = [[xywh[0] + xywh[2] / f(2), xywh[1] + xywh[3] / f(2), xywh[2], xywh[3], 0.0],
            [100.0, 100.0, 80.0, 20.0, 90.0], [50.5, 40.25, 30.0, 10.0, -35.0], [2.0, 5.0, 2.0, 8.0, 0.0]]
    _same(h["img_box5"], np.array(want, f))
    assert h["img_cls"].tolist() == [0, 1, 1, 1]
    _same(h["img_ratio5"], np.array([4.4 / 8.6, 20.0 / 80.0, 10.0 / 30.0, 0.3], np.float64).astype(f))      # ann 3: the explicit ratio
    assert gt.rotated_recall_arrays() is h
    # the segment-ordered arrays keep their five keys and their content
    r = gt.rotated_arrays()
    assert list(r) == ["seg_gt_off", "seg_box5", "seg_crowd", "seg_area", "seg_ratio5"]
    _same(r["seg_box5"], h["img_box5"])                  # this dataset's segment order happens to be its image order
    # the class goes through the metadata map
    assert CocoGt(ds, id_map={7: 0, 3: 1}).rotated_recall_arrays()["img_cls"].tolist() == [1, 0, 0, 0]


def test_rotated_recall_arrays_drop_crowd_and_ignore():
    ds = _four_ann_dataset()
    ds["annotations"][0]["ignore"] = 1                   # ann 1 (image 9): dropped although the dataset holds rotated boxes
    h = CocoGt(ds).rotated_recall_arrays()
    assert h["img_gt_off"].tolist() == [0, 2, 3] and h["img_cls"].tolist() == [0, 1, 1]
    _same(h["img_box5"][2], np.array([2.0, 5.0, 2.0, 8.0, 0.0], np.float32))
    ds["annotations"][1]["iscrowd"] = 1                  # a crowd gt beside five-number boxes: the error of rotated_arrays()
    with pytest.raises(ValueError):
        CocoGt(ds).rotated_recall_arrays()
    for a in ds["annotations"]:
        a["bbox"] = a["bbox"][:4]
    h = CocoGt(ds).rotated_recall_arrays()               # XYWH boxes only: the crowd gt (ann 2) and the ignored one (ann 1) are dropped
    assert h["img_gt_off"].tolist() == [0, 1, 2] and h["img_cls"].tolist() == [1, 1]
    _same(h["img_box5"], np.array([[140.0, 110.0, 80.0, 20.0, 0.0], [2.0, 5.0, 2.0, 8.0, 0.0]], np.float32))
    ds["annotations"][3]["bbox"] = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    with pytest.raises(ValueError):
        CocoGt(ds).rotated_recall_arrays()
    # an annotation of an unknown image takes no part; a dataset without annotations gives empty arrays
    ds = _four_ann_dataset()
    ds["annotations"][2]["image_id"] = 77
    assert CocoGt(ds).rotated_recall_arrays()["img_gt_off"].tolist() == [0, 2, 3]
    ds["annotations"] = []
    h = CocoGt(ds).rotated_recall_arrays()
    assert h["img_gt_off"].tolist() == [0, 0, 0] and h["img_box5"].shape == (0, 5) and h["img_cls"].shape == (0,)


# ------------------------------------------------------------------------------------------------ C ABI
def test_cabi_declares_the_rotated_recall_pass():
    from slenderobjdet_amd import _C
    from test_cabi_surface import _declared

    decl = _declared()
    assert decl["sod_proposal_ar_rotated_scratch_floats"] == 2 == len(_C._SIGS["sod_proposal_ar_rotated_scratch_floats"])
    assert decl["sod_proposal_ar_rotated"] == 23 == len(_C._SIGS["sod_proposal_ar_rotated"])
    assert decl["sod_proposal_ar_rotated"] == decl["sod_proposal_ar"] and _C._SIGS["sod_proposal_ar_rotated"] == _C._SIGS["sod_proposal_ar"]
    assert _C._RESTYPES["sod_proposal_ar_rotated_scratch_floats"] is ctypes.c_longlong


def test_scratch_size_query():
    from slenderobjdet_amd import _C

    lib = _C.load()
    q = lib.sod_proposal_ar_rotated_scratch_floats
    assert q(0, 100) == 0 and q(1, 100) == 0 and q(32, 100) == 0          # 32 * 100 = 3200 floats: both matrices in LDS
    assert q(33, 100) == 2 * 100 * 33 and q(300, 100) == 60000            # above: both [limit, G] matrices in the slot
    assert q(3201, 1) == 2 * 3201 and q(3200, 1) == 0
    assert q(-1, 100) == -1 and q(5, -1) == -1
    assert q(2 ** 31 - 1, 100) == 2 * 100 * (2 ** 31 - 1)                 # 64-bit arithmetic
    assert [q(g, 100) for g in (0, 32, 33, 300)] == [lib.sod_proposal_ar_scratch_floats(g, 100) for g in (0, 32, 33, 300)]


# ------------------------------------------------------------------------------------------------ angle 0: the axis-aligned pass
def angle0_fixture():
    """Integer-coordinate XYWH gts and XYXY predictions (dataset, preds in prediction order).  Every detection overlaps one gt only, by
    a shift that makes the edges cross; every positive IoU of an image has its own value.
      image 1  D > G; a detection of the wrong class covers gt 0 best: the class-agnostic and the class-aware rounds pick differently
      image 2  D < G
      image 3  two exact duplicate detections against one gt (the tie that is there by construction)
      image 4  gts, no detections;  image 5: detections, no gts - neither takes part"""
    gts = {1: [(1, (10, 10, 100, 18)), (2, (10, 100, 20, 100)), (1, (200, 10, 50, 50)), (2, (200, 200, 200, 100))],
           2: [(1, (20, 20, 60, 12)), (1, (20, 100, 60, 12)), (2, (300, 300, 40, 40))],
           3: [(2, (50, 50, 80, 16))],
           4: [(1, (5, 5, 30, 30))],
           5: []}
    # (image, contiguous class, XYWH): category 1 -> 0, 2 -> 1
    dets = [(1, 0, (12, 11, 100, 18)), (1, 1, (11, 10, 100, 18)), (1, 1, (11, 106, 20, 100)), (1, 0, (204, 12, 50, 50)),
            (1, 1, (220, 208, 200, 100)), (1, 0, (200, 235, 200, 100)), (1, 1, (290, 200, 200, 100)),
            (2, 0, (23, 21, 60, 12)), (2, 0, (22, 102, 60, 12)),
            (3, 1, (58, 51, 80, 16)), (3, 1, (58, 51, 80, 16)),
            (5, 0, (10, 10, 40, 40)), (5, 1, (60, 60, 20, 90))]
    images, anns = [], []
    for img, items in gts.items():
        images.append({"id": img, "width": 640, "height": 480})
        for c, b in items:
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": c, "bbox": [float(v) for v in b], "area": float(b[2] * b[3]),
                         "iscrowd": 0})
    ds = {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}]}
    xyxy = np.array([[x, y, x + w, y + h] for _, _, (x, y, w, h) in dets], np.float32)
    preds = {"image_id": np.array([d[0] for d in dets], np.int64), "category": np.array([d[1] for d in dets], np.int64), "boxes": xyxy,
             "score": np.linspace(0.9, 0.1, len(dets)).astype(np.float32)}
    return ds, preds


def restated_inputs(ds, preds):
    """(gt index, gts by image with ratio and box5, images of the axis-aligned restatement (XYWH), images of the rotated one (box5))."""
    gt = CocoGt(ds)
    gt.rotated_arrays()                                  # raises for what the rotated evaluator refuses
    by_img = {}
    for a in gt.anns:
        w, hh = float(a["bbox"][2]), float(a["bbox"][3])
        ratio = float(a["ratio"]) if "ratio" in a else (min(w, hh) / max(w, hh) if max(w, hh) > 0 else 0.0)
        crowd = int(bool(a.get("iscrowd", 0) or a.get("ignore", 0)))
        by_img.setdefault(a["image_id"], []).append(dict(a, ratio=ratio, box5=RR.gt_box5(a["bbox"]), iscrowd=crowd))
    b = np.asarray(preds["boxes"], np.float32)
    box5 = RR.pred_box5(b) if len(b) else np.zeros((0, 5), np.float32)
    xywh = np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], axis=1) if b.shape[1] == 4 else None
    images4, images5, seen = [], [], []
    for img in preds["image_id"].tolist():
        if img in seen:
            continue
        seen.append(img)
        sel = np.nonzero(preds["image_id"] == img)[0]
        images5.append((img, box5[sel], preds["category"][sel]))
        if xywh is not None:
            images4.append((img, xywh[sel], preds["category"][sel]))
    return gt, by_img, images4, images5


def assert_fixture_condition(by_img, images5, id_map, limit=100):
    """In float64: every IoU at least 1e-3 away from each of the ten thresholds, and in every round of both matrices the maximum at
    least 1e-3 above every other remaining entry that is not its exact duplicate by construction (an equal row in the same column,
    an equal column in the same row)."""
    thr = 0.5 + 0.05 * np.arange(10)
    rounds = 0
    for img, boxes, classes in images5:
        anno = [o for o in by_img.get(img, []) if o["iscrowd"] == 0]
        if not anno or not len(boxes):
            continue
        d = np.asarray(boxes[:limit], np.float64)
        g = np.stack([o["box5"] for o in anno]).astype(np.float64)
        D, G = len(d), len(g)
        iou = RL.iou(torch.from_numpy(np.repeat(d, G, axis=0)), torch.from_numpy(np.tile(g, (D, 1)))).numpy().reshape(D, G)
        assert np.abs(iou[..., None] - thr).min() >= 1e-3, (img, iou)
        same = np.array([[int(c) == id_map[o["category_id"]] for o in anno] for c in classes[:limit]], np.float64)
        for m in (iou.copy(), iou * same):
            for _ in range(min(D, G)):
                gi = int(np.argmax(m.max(axis=0)))
                di = int(np.argmax(m[:, gi]))
                best = m[di, gi]
                assert best > 0
                for i in range(D):
                    for j in range(G):
                        dup = (i == di or np.array_equal(d[i], d[di])) and (j == gi or np.array_equal(g[j], g[gi]))
                        assert dup or best - m[i, j] >= 1e-3, (img, di, gi, i, j, best, m[i, j])
                m[di, :] = -1
                m[:, gi] = -1
                rounds += 1
    return rounds


def test_angle0_restatement_equals_axis_aligned_restatement():
    ds, preds = angle0_fixture()
    gt, by_img, images4, images5 = restated_inputs(ds, preds)
    assert assert_fixture_condition(by_img, images5, gt.id_map) == 2 * (4 + 2 + 1)
    want, ar_w, mar_w, num_pos_w, used_w = RS.proposal_ar(images4, by_img, gt.id_map, len(gt.cat_ids))
    got, ar, mar, num_pos, used, hits = AR.proposal_ar_rotated(images5, by_img, gt.id_map, len(gt.cat_ids), RR.oracle_iou)
    assert used == used_w == 3
    _same(num_pos.numpy(), num_pos_w.numpy())
    _same(got.numpy(), want.numpy())
    assert float(ar) == float(ar_w) and float(mar) == float(mar_w)
    # the fixture shows what it is there for: the two matrices disagree on gt 0 of image 1 (IoU 99 / 101 by the wrong class against 0.861 by class "a")
    assert int(num_pos[-1, 0, 0]) == 8 and int(hits[0, -1, 0, 0]) == 7
    assert int(hits[-1, -1, 0, 0]) > int(hits[-1, 0, 0, 0]) + int(hits[-1, 1, 0, 0])


# ------------------------------------------------------------------------------------------------ result dict
def test_results_dict_has_the_axis_aligned_keys():
    ds, preds = angle0_fixture()
    gt, by_img, images4, images5 = restated_inputs(ds, preds)
    recalls, ar, mar, num_pos, _, _ = AR.proposal_ar_rotated(images5, by_img, gt.id_map, len(gt.cat_ids), RR.oracle_iou)
    want = RS.ar_results(*RS.proposal_ar(images4, by_img, gt.id_map, len(gt.cat_ids))[:4])
    res = ar_results(recalls, num_pos)
    st = res.pop("ar-stats")
    assert list(res) == list(want) == list(AR.ar_results(recalls, ar, mar, num_pos)) and len(res) == 22
    assert res == want
    assert list(st) == ["ar", "mar", "thresholds", "gt_overlaps", "num_pos"]
