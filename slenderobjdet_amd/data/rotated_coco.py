"""Rotated ground truth from polygons: what the reference's tools/mask_to_rbox.py (:40-60, over COCO.compute_rbox and
concern.support.rbox_from_polygon) writes into the rbox_{train,val}2017.json files behind its rcoco_2017_* datasets, with the
rectangles of all annotations from one call of structures.polygons.min_area_rects instead of one OpenCV call each.

Kept, not fixed: a crowd annotation that is not skipped becomes [x, y, w, h, 0] - the XYWH box's top-left corner stands where the
five-number form has the centre, exactly as compute_rbox writes it."""
import copy
import datetime


def coco_to_rotated(dataset, skip_crowd=False, device="cpu"):
    """A COCO dict (the input is not modified) whose every ``bbox`` holds five numbers (cx, cy, w, h, angle_deg): the canonical
    minimum-area rectangle of a non-crowd annotation's polygons; a crowd annotation is dropped when ``skip_crowd`` (the reference does
    so for val files) and becomes [x, y, w, h, 0] otherwise.  Raises ValueError for a non-crowd annotation without a usable polygon
    (the reference asserts).  ``images`` and ``categories`` are copied through."""
    from ..evaluation.coco_gt import load_json      # here, not at the top: evaluation imports data.catalog
    from ..structures.polygons import min_area_rects, pack_polygons, usable_polygons

    dataset = load_json(dataset)
    src = dataset.get("annotations", [])
    for ann in src:
        if not ann.get("iscrowd", 0) and not usable_polygons(ann):
            raise ValueError(f"annotation {ann.get('id')} is not a crowd and has no usable polygon (an even number >= 6 of coordinates)")
    xy, off, index = pack_polygons(src)
    rect, _ = min_area_rects(xy, off, device)
    box_of = {int(i): [float(v) for v in rect[j]] for j, i in enumerate(index)}
    anns = []
    for i, ann in enumerate(src):
        if ann.get("iscrowd", 0):
            if skip_crowd:
                continue
            box = [*ann["bbox"][:4], 0]
        else:
            box = box_of[i]
        ann = copy.copy(ann)
        ann["bbox"] = box
        anns.append(ann)
    info = dict(date_created=str(datetime.datetime.now()),
                description="Rotated-box (cx, cy, w, h, angle_deg) version of a polygon dataset: minimum-area rectangles of the polygons.")
    return dict(info=info, categories=dataset.get("categories", []), annotations=anns, images=dataset.get("images", []), license=None)


__all__ = ["coco_to_rotated"]
