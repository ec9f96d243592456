"""COCO-format ground truth for the evaluator: the json read with the standard library, the gt aspect ratio of
slender_det/evaluation/coco.py:61-84 (oriented=True), and the flat per-segment arrays the HIP kernels read.

Ratio rules (first that applies): an explicit ``"ratio"`` field; a crowd gt or one without a usable polygon (a polygon needs an
even number >= 6 of coordinates) takes min(w, h) / max(w, h) of its bbox; otherwise the side ratio min / max of the minimum-area
rectangle around the convex hull of all its polygons' points (0 for a degenerate rectangle).  The reference computes that rectangle
with OpenCV; it is restated here in numpy (monotone-chain hull + rotating calipers).
"""
import json

import numpy as np


def load_json(json_file):
    if isinstance(json_file, dict):
        return json_file
    with open(json_file) as f:
        return json.load(f)


def _hull(pts):
    """Convex hull (counter-clockwise, no collinear points) of [n, 2] float64 points."""
    pts = np.unique(pts, axis=0)
    if len(pts) < 3:
        return pts
    pts = pts[np.lexsort((pts[:, 1], pts[:, 0]))]

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in pts[::-1]:
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.array(lower[:-1] + upper[:-1])


def min_area_rect_sides(pts):
    """(w, h) of the minimum-area enclosing rectangle of [n, 2] points: one of its sides lies on a hull edge."""
    hull = _hull(np.asarray(pts, np.float64).reshape(-1, 2))
    if len(hull) < 3:
        return None
    best = None
    for i in range(len(hull)):
        e = hull[(i + 1) % len(hull)] - hull[i]
        n = np.hypot(e[0], e[1])
        if n == 0:
            continue
        u = e / n
        v = np.array([-u[1], u[0]])
        pu, pv = hull @ u, hull @ v
        w, h = pu.max() - pu.min(), pv.max() - pv.min()
        if best is None or w * h < best[0] * best[1]:
            best = (w, h)
    return best


def _ratio_of_box(w, h):
    if w * h == 0:
        return 0.0
    return min(w, h) / max(w, h)


def polygon_ratio(polygons):
    pts = np.concatenate([np.asarray(p, np.float64) for p in polygons]).reshape(-1, 2)
    wh = min_area_rect_sides(pts)
    if wh is None:       # fewer than 3 hull points: the axis-aligned extent
        return _ratio_of_box(pts[:, 0].max() - pts[:, 0].min(), pts[:, 1].max() - pts[:, 1].min())
    return _ratio_of_box(*wh)


def gt_ratio(ann):
    if "ratio" in ann:
        return ann["ratio"]
    seg = ann.get("segmentation")
    polys = [p for p in seg if len(p) % 2 == 0 and len(p) >= 6] if isinstance(seg, list) else []
    if ann["iscrowd"] or "segmentation" not in ann or len(polys) == 0:
        w, h = ann["bbox"][2], ann["bbox"][3]
        return min(w, h) / max(w, h)
    return polygon_ratio(polys)


class CocoGt:
    """Index of a COCO-format dataset: sorted image and category ids, every annotation with its ratio, and the category maps."""

    def __init__(self, dataset, id_map=None, class_names=None, ratio_device=None):
        """ratio_device: None computes every ratio with the host loop above; a device ("cuda", "cpu") takes the ratios of all annotations
        from structures.polygons.oriented_ratios - one kernel launch on a GPU - by the same rules."""
        self.dataset = load_json(dataset)
        self.img_ids = sorted({im["id"] for im in self.dataset.get("images", [])})
        cats = self.dataset.get("categories", [])
        self.cat_ids = sorted(c["id"] for c in cats)
        self.cats = {c["id"]: c for c in cats}
        # dataset category id -> contiguous id: the metadata's map, else the identity order over the sorted ids
        self.id_map = dict(id_map) if id_map is not None else {c: i for i, c in enumerate(self.cat_ids)}
        self.class_names = list(class_names) if class_names is not None else None
        self.has_annotations = "annotations" in self.dataset
        self.anns = list(self.dataset.get("annotations", []))
        if ratio_device is None:
            self.ratios = np.array([float(gt_ratio(a)) for a in self.anns], np.float64)
        else:
            from ..structures.polygons import oriented_ratios

            self.ratios = oriented_ratios(self.anns, ratio_device)
        self._arrays = None
        self._rotated_arrays = None
        self._rotated_recall_arrays = None

    def _segment_order(self):
        """(image index of every annotation or -1, the annotations of known images and categories ordered by (category, image)
        segment and json order within, seg_gt_off [K*I+1])."""
        I, K = len(self.img_ids), len(self.cat_ids)
        img_idx = {im: i for i, im in enumerate(self.img_ids)}
        cat_idx = {c: k for k, c in enumerate(self.cat_ids)}
        img_of = np.array([img_idx.get(a["image_id"], -1) for a in self.anns], np.int64)
        cat_of = np.array([cat_idx.get(a["category_id"], -1) for a in self.anns], np.int64)
        keep = (img_of >= 0) & (cat_of >= 0)
        seg = cat_of * I + img_of
        order = np.nonzero(keep)[0]
        order = order[np.argsort(seg[order], kind="stable")]
        seg_gt_off = np.zeros(K * I + 1, np.int32)
        np.cumsum(np.bincount(seg[order], minlength=K * I), out=seg_gt_off[1:])
        return img_of, order, seg_gt_off

    def arrays(self):
        """Flat numpy arrays of the kernels' gt side (cached):
        seg_gt_off [K*I+1] / seg_box [G,4] f64 / seg_crowd [G] u8 / seg_ratio [G] f64 - gts by (category, image) segment in json order;
        img_gt_off [I+1] / img_box [G',4] f32 / img_cls [G'] i32 / img_ratio [G'] f32 - non-crowd gts by image for the recall pass."""
        if self._arrays is not None:
            return self._arrays
        I = len(self.img_ids)
        n = len(self.anns)
        img_of, order, seg_gt_off = self._segment_order()
        box = np.array([a["bbox"][:4] for a in self.anns], np.float64).reshape(n, 4)
        crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in self.anns], np.uint8)
        # recall pass: the non-crowd gts of each image, class mapped through the metadata map
        ar_keep = np.nonzero((img_of >= 0) & (np.array([a["iscrowd"] == 0 for a in self.anns], bool) if n else np.zeros(0, bool)))[0]
        ar_keep = ar_keep[np.argsort(img_of[ar_keep], kind="stable")]
        img_gt_off = np.zeros(I + 1, np.int32)
        np.cumsum(np.bincount(img_of[ar_keep], minlength=I), out=img_gt_off[1:])
        img_cls = np.array([self.id_map[self.anns[j]["category_id"]] for j in ar_keep], np.int32)
        self._arrays = dict(
            seg_gt_off=seg_gt_off, seg_box=np.ascontiguousarray(box[order]), seg_crowd=crowd[order], seg_ratio=self.ratios[order],
            img_gt_off=img_gt_off, img_box=box[ar_keep].astype(np.float32), img_cls=img_cls,
            img_ratio=self.ratios[ar_keep].astype(np.float32),
        )
        return self._arrays

    def rotated_arrays(self):
        """The gt side of the rotated-box evaluation (detectron2's RotatedCOCOeval), in the segment order of arrays() (cached):
        seg_gt_off [K*I+1] / seg_box5 [G,5] f32 (cx, cy, w, h, angle_deg) / seg_crowd [G] u8 / seg_area [G] f64 / seg_ratio5 [G] f64.
        A five-number ``bbox`` is taken as it is; an XYWH one becomes (x + w/2, y + h/2, w, h, 0) in float32.  seg_area is the
        annotation's ``area``, else w * h; seg_ratio5 an explicit ``ratio``, else min(w, h) / max(w, h) of the box.  Raises
        ValueError for a dataset that holds both a five-number box and a crowd gt: the rotated IoU has no crowd form."""
        if self._rotated_arrays is not None:
            return self._rotated_arrays
        _, order, seg_gt_off = self._segment_order()
        box5, area, ratio, crowd = self._rotated_boxes()
        self._rotated_arrays = dict(seg_gt_off=seg_gt_off, seg_box5=np.ascontiguousarray(box5[order]), seg_crowd=crowd[order],
                                    seg_area=area[order], seg_ratio5=ratio[order])
        return self._rotated_arrays

    def _rotated_boxes(self):
        """Per annotation in json order: box5 [n, 5] f32, area [n] f64, ratio [n] f64, crowd [n] u8 (``iscrowd`` or ``ignore``) by the
        rules of rotated_arrays(), whose errors it raises."""
        n = len(self.anns)
        five = [len(a["bbox"]) == 5 for a in self.anns]
        if any(len(a["bbox"]) not in (4, 5) for a in self.anns):
            raise ValueError("a bbox must hold 4 (XYWH) or 5 (cx, cy, w, h, angle) numbers")
        if any(five) and any(a.get("iscrowd", 0) for a in self.anns):
            raise ValueError("a dataset with rotated (five-number) boxes must not hold crowd annotations")
        box5 = np.zeros((n, 5), np.float32)
        area = np.zeros(n, np.float64)
        ratio = np.zeros(n, np.float64)
        for j, a in enumerate(self.anns):
            b = np.array(a["bbox"], np.float32)
            if five[j]:
                box5[j] = b
            else:
                box5[j] = (b[0] + b[2] / np.float32(2), b[1] + b[3] / np.float32(2), b[2], b[3], 0)
            w, h = float(a["bbox"][2]), float(a["bbox"][3])
            area[j] = float(a["area"]) if "area" in a else w * h
            ratio[j] = float(a["ratio"]) if "ratio" in a else (min(w, h) / max(w, h) if max(w, h) > 0 else 0.0)
        crowd = np.array([1 if (a.get("iscrowd", 0) or a.get("ignore", 0)) else 0 for a in self.anns], np.uint8)
        return box5, area, ratio, crowd

    def rotated_recall_arrays(self):
        """The gt side of the rotated recall pass (cached): the non-crowd gts (neither ``iscrowd`` nor ``ignore``) of the known images,
        ordered by image and in json order within one -
        img_gt_off [I+1] i32 / img_box5 [G', 5] f32 / img_cls [G'] i32 contiguous ids through the metadata map / img_ratio5 [G'] f32.
        Boxes and ratios by the rules of rotated_arrays(), whose errors it raises."""
        if self._rotated_recall_arrays is not None:
            return self._rotated_recall_arrays
        I = len(self.img_ids)
        img_idx = {im: i for i, im in enumerate(self.img_ids)}
        img_of = np.array([img_idx.get(a["image_id"], -1) for a in self.anns], np.int64)
        box5, _, ratio, crowd = self._rotated_boxes()
        keep = np.nonzero((img_of >= 0) & (crowd == 0))[0]
        keep = keep[np.argsort(img_of[keep], kind="stable")]
        img_gt_off = np.zeros(I + 1, np.int32)
        np.cumsum(np.bincount(img_of[keep], minlength=I), out=img_gt_off[1:])
        img_cls = np.array([self.id_map[self.anns[j]["category_id"]] for j in keep], np.int32)
        self._rotated_recall_arrays = dict(img_gt_off=img_gt_off, img_box5=np.ascontiguousarray(box5[keep]), img_cls=img_cls,
                                           img_ratio5=ratio[keep].astype(np.float32))
        return self._rotated_recall_arrays
