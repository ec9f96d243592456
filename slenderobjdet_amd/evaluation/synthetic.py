"""Synthetic COCO-format ground truth + scored detections for the evaluation tests and tools/bench_coco_eval.py (there is no
dataset on the box).  Gts follow data/synthetic.py (Poisson(7) boxes per image, log-uniform 16..600 px sides, 20 % slender
1:5 .. 1:10); detections are jittered copies of the gts plus background boxes, with float32 scores.

Returns ``(dataset, preds)``: ``dataset`` a COCO json dict (images / annotations / categories, non-contiguous ids in shuffled
json order) and ``preds`` a dict of numpy arrays in prediction order: image_id int64, category (contiguous id) int64,
boxes [N, 4] XYXY float32, score float32 - the flattened per-image ``Instances`` of a detector.  ``synthetic_rotated_coco`` is the
same for (cx, cy, w, h, angle_deg) boxes.
"""
import numpy as np


def synthetic_coco(seed, n_images=40, n_cats=6, dets_per_image=(0, 30), slender=0.2, crowd=0.05, no_gt=0.1, no_dt=0.1,
                   width=640, height=480, score_levels=None, dup=0.0, max_gts=50):
    """``dets_per_image`` (lo, hi): detections per image uniform in [lo, hi]; ``score_levels`` > 0 draws scores from that many
    distinct values (ties within and across images); ``dup`` the fraction of detections repeated with the same box and score."""
    rs = np.random.RandomState(seed)
    cat_ids = sorted(rs.choice(np.arange(1, 3 * n_cats + 1), n_cats, replace=False).tolist())
    img_ids = rs.choice(np.arange(1, 100 * n_images + 1), n_images, replace=False).tolist()   # json order is not id order
    cats = [{"id": int(c), "name": f"cat{c}"} for c in rs.permutation(cat_ids)]
    images, anns = [], []
    pi, pc, pb, ps = [], [], [], []
    ann_id = 1
    for img in img_ids:
        images.append({"id": int(img), "width": width, "height": height})
        G = 0 if rs.rand() < no_gt else int(np.clip(rs.poisson(7), 1, max_gts))
        w = 2.0 ** (rs.rand(G) * 5.2 + 4.0)
        h = 2.0 ** (rs.rand(G) * 5.2 + 4.0)
        sl = rs.rand(G) < slender
        r = rs.randint(5, 11, G).astype(np.float64)
        tall = rs.rand(G) < 0.5
        h = np.where(sl & tall, w * r, h)
        w = np.where(sl & ~tall, h * r, w)
        x = np.clip(rs.rand(G) * width - w / 2, 0, width - 2)
        y = np.clip(rs.rand(G) * height - h / 2, 0, height - 2)
        w = np.maximum(np.minimum(w, width - x), 2.0)
        h = np.maximum(np.minimum(h, height - y), 2.0)
        cls = rs.randint(0, n_cats, G)
        gts = []
        for j in range(G):
            box = [round(float(x[j]), 2), round(float(y[j]), 2), round(float(w[j]), 2), round(float(h[j]), 2)]
            a = {"id": ann_id, "image_id": int(img), "category_id": int(cat_ids[cls[j]]), "bbox": box,
                 "area": box[2] * box[3], "iscrowd": int(rs.rand() < crowd)}
            ann_id += 1
            anns.append(a)
            gts.append((box, int(cls[j])))
        if rs.rand() < no_dt:
            continue
        D = rs.randint(dets_per_image[0], dets_per_image[1] + 1)
        for _ in range(D):
            if gts and rs.rand() < 0.7:
                box, c = gts[rs.randint(len(gts))]
                jit = rs.randn(4) * 0.08 * np.array([box[2], box[3], box[2], box[3]])
                x1, y1 = box[0] + jit[0], box[1] + jit[1]
                x2, y2 = box[0] + box[2] + jit[2], box[1] + box[3] + jit[3]
                if rs.rand() < 0.15:
                    c = rs.randint(n_cats)
            else:
                c = rs.randint(n_cats)
                x1, y1 = rs.rand() * width, rs.rand() * height
                x2, y2 = x1 + 2.0 ** (rs.rand() * 6 + 3), y1 + 2.0 ** (rs.rand() * 6 + 3)
            x1, x2 = np.clip(x1, 0, width), np.clip(x2, 0, width)
            y1, y2 = np.clip(y1, 0, height), np.clip(y2, 0, height)
            if x2 - x1 < 1:
                x2 = min(x1 + 1.0, width)
                x1 = x2 - 1.0
            if y2 - y1 < 1:
                y2 = min(y1 + 1.0, height)
                y1 = y2 - 1.0
            s = rs.randint(1, score_levels + 1) / score_levels if score_levels else rs.rand()
            n = 2 if rs.rand() < dup else 1
            for _ in range(n):
                pi.append(img)
                pc.append(c)
                pb.append([x1, y1, x2, y2])
                ps.append(s)
    dataset = {"images": images, "annotations": anns, "categories": cats}
    preds = {"image_id": np.array(pi, np.int64), "category": np.array(pc, np.int64),
             "boxes": np.array(pb, np.float32).reshape(-1, 4), "score": np.array(ps, np.float32)}
    return dataset, preds


def synthetic_rotated_coco(seed, n_images=40, n_cats=6, dets_per_image=(0, 30), slender=0.2, no_gt=0.1, no_dt=0.1, width=640,
                           height=480, score_levels=None, dup=0.0, max_gts=50):
    """The recipe of ``synthetic_coco`` for rotated boxes: every gt is (cx, cy, w, h, angle_deg) with the angle uniform in
    (-90, 90], ``area`` = w * h and no crowd gts; a detection is a jittered gt (centre and size by 8 %, the angle by a few
    degrees) or a background box.  ``preds["boxes"]`` is [N, 5] float32."""
    rs = np.random.RandomState(seed)
    cat_ids = sorted(rs.choice(np.arange(1, 3 * n_cats + 1), n_cats, replace=False).tolist())
    img_ids = rs.choice(np.arange(1, 100 * n_images + 1), n_images, replace=False).tolist()   # json order is not id order
    cats = [{"id": int(c), "name": f"cat{c}"} for c in rs.permutation(cat_ids)]
    images, anns = [], []
    pi, pc, pb, ps = [], [], [], []
    ann_id = 1
    for img in img_ids:
        images.append({"id": int(img), "width": width, "height": height})
        G = 0 if rs.rand() < no_gt else int(np.clip(rs.poisson(7), 1, max_gts))
        w = 2.0 ** (rs.rand(G) * 5.2 + 4.0)
        h = 2.0 ** (rs.rand(G) * 5.2 + 4.0)
        sl = rs.rand(G) < slender
        r = rs.randint(5, 11, G).astype(np.float64)
        tall = rs.rand(G) < 0.5
        h = np.minimum(np.where(sl & tall, w * r, h), 600.0)
        w = np.minimum(np.where(sl & ~tall, h * r, w), 600.0)
        cx, cy = rs.rand(G) * width, rs.rand(G) * height
        ang = 90.0 - rs.rand(G) * 180.0
        cls = rs.randint(0, n_cats, G)
        gts = []
        for j in range(G):
            box = [round(float(cx[j]), 2), round(float(cy[j]), 2), round(float(w[j]), 2), round(float(h[j]), 2), round(float(ang[j]), 2)]
            anns.append({"id": ann_id, "image_id": int(img), "category_id": int(cat_ids[cls[j]]), "bbox": box,
                         "area": box[2] * box[3], "iscrowd": 0})
            ann_id += 1
            gts.append((box, int(cls[j])))
        if rs.rand() < no_dt:
            continue
        D = rs.randint(dets_per_image[0], dets_per_image[1] + 1)
        for _ in range(D):
            if gts and rs.rand() < 0.7:
                box, c = gts[rs.randint(len(gts))]
                jit = rs.randn(4) * 0.08 * np.array([box[2], box[3], box[2], box[3]])
                b = [box[0] + jit[0], box[1] + jit[1], max(box[2] + jit[2], 1.0), max(box[3] + jit[3], 1.0), box[4] + rs.randn() * 4.0]
                if rs.rand() < 0.15:
                    c = rs.randint(n_cats)
            else:
                c = rs.randint(n_cats)
                b = [rs.rand() * width, rs.rand() * height, 2.0 ** (rs.rand() * 6 + 3), 2.0 ** (rs.rand() * 6 + 3), 90.0 - rs.rand() * 180.0]
            s = rs.randint(1, score_levels + 1) / score_levels if score_levels else rs.rand()
            n = 2 if rs.rand() < dup else 1
            for _ in range(n):
                pi.append(img)
                pc.append(c)
                pb.append(b)
                ps.append(s)
    dataset = {"images": images, "annotations": anns, "categories": cats}
    preds = {"image_id": np.array(pi, np.int64), "category": np.array(pc, np.int64),
             "boxes": np.array(pb, np.float32).reshape(-1, 5), "score": np.array(ps, np.float32)}
    return dataset, preds


def preds_xywh(preds):
    """XYXY -> XYWH in float32, as detectron2's instances_to_coco_json does."""
    b = preds["boxes"].astype(np.float32)
    out = b.copy()
    out[:, 2] = b[:, 2] - b[:, 0]
    out[:, 3] = b[:, 3] - b[:, 1]
    return out
