"""Minimum-area rectangles of polygon annotations: the rectangle behind the reference's oriented ratio (COCO.compute_ratio,
PolygonMasks.get_ratios(oriented=True), concern.support.ratio_of_polygon) and its rotated ground truth (COCO.compute_rbox,
concern.support.rbox_from_polygon), for all annotations of a dataset in one launch of csrc/polygon_geom.hip.

Per annotation (its points are those of all its usable polygons): the convex hull of the distinct points, counter-clockwise from the
lexicographically smallest (x, y) point; for every hull edge with unit direction u and normal v = (-uy, ux) the extents w along u and h
along v; the edge of least w * h, the first one in hull order among equal areas (an acute triangle has three); centre
u * mid_u + v * mid_v; angle degrees(atan2(-uy, ux)) - detectron2's convention, the width axis is (cos a, -sin a) in image coordinates -
folded into (-45, 45] by multiples of 90 with w and h swapped for an odd multiple, the form rbox_from_polygon leaves.  Fewer than three
hull vertices (one point, coincident or collinear points) give the axis-aligned extent with angle 0 and ``info < 3``.

Deviations from the reference, which calls OpenCV on float32 copies: float64 from the json numbers throughout; the degenerate rule
(OpenCV returns a zero-width rotated rectangle there); the deterministic tie rule (OpenCV's choice among equal areas follows its
rotating-calipers order and float32 rounding).

``device="cpu"`` runs a float64 numpy path with the kernel's arithmetic, operation by operation; a GPU device runs the kernel.
"""
import ctypes
import math

import numpy as np

LDS_POINTS = 512          # SOD_POLYGON_LDS_POINTS: larger annotations are read from global memory by the kernel
MAX_POINTS = 1 << 20      # SOD_POLYGON_MAX_POINTS per annotation
MAX_ANNS = 1 << 24        # SOD_POLYGON_MAX_ANNS per call
_DEG = 57.29577951308232  # 180 / pi, the kernel's constant


def usable_polygons(ann):
    """The polygons of an annotation the reference keeps: lists of an even number >= 6 of coordinates ([] for RLE or none)."""
    seg = ann.get("segmentation")
    if not isinstance(seg, list):
        return []
    return [p for p in seg if len(p) % 2 == 0 and len(p) >= 6]


def pack_polygons(anns):
    """(xy float64 [P, 2], ann_off int32 [A' + 1], index int64 [A']): the points of every non-crowd annotation with a usable polygon,
    flattened in order; index[j] is the position in ``anns`` of packed annotation j."""
    chunks, counts, index = [], [], []
    for i, ann in enumerate(anns):
        if ann.get("iscrowd", 0):
            continue
        polys = usable_polygons(ann)
        if not polys:
            continue
        n = 0
        for p in polys:
            chunks.append(p)
            n += len(p) // 2
        counts.append(n)
        index.append(i)
    xy = np.concatenate([np.asarray(c, np.float64) for c in chunks]).reshape(-1, 2) if chunks else np.zeros((0, 2), np.float64)
    if len(xy) >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 polygon points: split the annotations over several calls")
    ann_off = np.zeros(len(counts) + 1, np.int32)
    np.cumsum(np.asarray(counts, np.int64), out=ann_off[1:])
    return xy, ann_off, np.asarray(index, np.int64)


def _fold_angle(a, w, h):
    """The unique angle in (-45, 45] congruent to ``a`` modulo 90, and (w, h) swapped for an odd multiple."""
    k = int(math.ceil((a - 45.0) / 90.0))
    a -= 90.0 * k
    if a > 45.0:
        a -= 90.0
        k += 1
    elif a <= -45.0:
        a += 90.0
        k -= 1
    if k & 1:
        w, h = h, w
    return a + 0.0, w, h


def _min_area_rect_host(pts):
    """One annotation on the host: ((cx, cy, w, h, angle_deg), hull vertices)."""
    from ..evaluation.coco_gt import _hull

    hull = _hull(pts)
    if len(hull) < 3:
        lox, loy = pts.min(axis=0)
        hix, hiy = pts.max(axis=0)
        return ((lox + hix) / 2, (loy + hiy) / 2, hix - lox, hiy - loy, 0.0), len(hull)
    e = np.roll(hull, -1, axis=0) - hull
    length = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    ux, uy = e[:, 0] / length, e[:, 1] / length
    x, y = hull[:, 0][:, None], hull[:, 1][:, None]
    pu = x * ux + y * uy              # [vertex, edge]; elementwise: no BLAS, no fused multiply-add
    pv = y * ux - x * uy
    lou, hiu, lov, hiv = pu.min(axis=0), pu.max(axis=0), pv.min(axis=0), pv.max(axis=0)
    i = int(np.argmin((hiu - lou) * (hiv - lov)))     # the first minimal edge
    mu, mv = (lou[i] + hiu[i]) / 2, (lov[i] + hiv[i]) / 2
    a = math.atan2(-uy[i], ux[i]) * _DEG
    a, w, h = _fold_angle(a, hiu[i] - lou[i], hiv[i] - lov[i])
    return (ux[i] * mu - uy[i] * mv, uy[i] * mu + ux[i] * mv, w, h, a), len(hull)


def _check_packed(xy, ann_off):
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    off = np.ascontiguousarray(ann_off, np.int64).reshape(-1)
    if len(off) < 1 or off[0] != 0 or off[-1] != len(xy):
        raise ValueError("ann_off must run from 0 to the number of points")
    n = np.diff(off)
    if len(n) > MAX_ANNS:
        raise ValueError(f"{len(n)} annotations in one call (at most {MAX_ANNS})")
    if len(n) and (n.min() < 1 or n.max() > MAX_POINTS):
        raise ValueError(f"every annotation needs between 1 and {MAX_POINTS} points")
    if len(xy) >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 polygon points in one call")
    return xy, off.astype(np.int32)


def min_area_rects(xy, ann_off, device="cpu"):
    """(rect float64 [A, 5] = (cx, cy, w, h, angle_deg), info int32 [A] = hull vertices, < 3 for the degenerate rule) of the packed
    annotations.  A GPU ``device`` costs one host-to-device copy, one launch and one device-to-host copy."""
    import torch

    xy, off = _check_packed(xy, ann_off)
    A = len(off) - 1
    dev = torch.device(device)
    if dev.type == "cpu":
        rect = np.zeros((A, 5), np.float64)
        info = np.zeros(A, np.int32)
        for a in range(A):
            rect[a], info[a] = _min_area_rect_host(xy[off[a]:off[a + 1]])
        return rect, info
    from .. import _C

    # one buffer each way: the points (16-byte aligned) and the offsets behind them; the rectangles and the hull sizes behind them
    host = np.empty(16 * len(xy) + 4 * (A + 1), np.uint8)
    host[:16 * len(xy)] = xy.view(np.uint8).reshape(-1)
    host[16 * len(xy):] = off.view(np.uint8)
    with torch.cuda.device(dev):
        d_in = torch.from_numpy(host).to(dev)
        d_out = torch.empty(44 * A, dtype=torch.uint8, device=dev)
        _C.call("sod_polygon_min_area_rect", ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_in.data_ptr() + 16 * len(xy)), A,
                ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(d_out.data_ptr() + 40 * A), _C.stream_ptr())
        out = d_out.cpu().numpy()
    return out[:40 * A].view(np.float64).reshape(A, 5).copy(), out[40 * A:].view(np.int32).copy()


def oriented_ratios(anns, device="cpu"):
    """float64 [len(anns)]: the gt aspect ratio of every annotation by the rules of evaluation/coco_gt.py - an explicit ``"ratio"``;
    the bbox ratio min(w, h) / max(w, h) for a crowd gt or one without a usable polygon; else min(w, h) / max(w, h) of the
    minimum-area rectangle of its polygons, 0 when w * h == 0 - with all rectangles from one min_area_rects call."""
    out = np.zeros(len(anns), np.float64)
    xy, off, index = pack_polygons(anns)
    packed = np.zeros(len(anns), bool)
    packed[index] = True
    for i, ann in enumerate(anns):
        if "ratio" in ann:
            out[i] = ann["ratio"]
            packed[i] = False
        elif not packed[i]:
            w, h = ann["bbox"][2], ann["bbox"][3]
            out[i] = min(w, h) / max(w, h)
    if len(index):
        rect, _ = min_area_rects(xy, off, device)
        w, h = rect[:, 2], rect[:, 3]
        big = np.maximum(w, h)
        r = np.where(w * h == 0, 0.0, np.minimum(w, h) / np.where(big == 0, 1.0, big))
        use = packed[index]
        out[index[use]] = r[use]
    return out


__all__ = ["LDS_POINTS", "MAX_ANNS", "MAX_POINTS", "min_area_rects", "oriented_ratios", "pack_polygons", "usable_polygons"]
