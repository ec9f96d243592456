"""Rotated-box IoU restated in float64 torch for the tests of the rotated IoU loss (layers.rotated_iou_loss, sod_rotated_iou_loss,
sod_retina_riou_loss_*): a helper, not reference code.

  iou(a, b)       boxes (P, 5) = (cx, cy, w, h, angle_deg), detectron2's axes: width along (cos t, -sin t), height along (sin t, cos t).
                  The rectangle ``a`` is carried into the frame of ``b`` and clipped against b's four half planes (Sutherland-Hodgman on
                  fixed 8-slot vertex lists, all pairs at once); the area is the shoelace sum.  Every step is a differentiable torch
                  operation, so autograd gives d IoU / d a - by another route than the kernel's boundary integral.
  margin(a, b)    the smallest distance between a vertex of one rectangle and an edge (segment) of the other, 32 pairs: the structure of
                  the intersection polygon changes exactly where this is 0, and the IoU has a kink there.
  generate(n, s)  the random pairs of the tests: slender gts and jittered predictions.
  special_cases() the hand-made pairs; ``forward_only`` marks those that sit on a kink (identical rectangles).
"""
import math

import torch

F64 = torch.float64


def _axes(t_deg):
    t = t_deg * (math.pi / 180.0)
    c, s = torch.cos(t), torch.sin(t)
    return torch.stack([c, -s], -1), torch.stack([s, c], -1)          # width axis, height axis


def vertices(b):
    """(P, 5) -> (P, 4, 2) in the order of detectron2's get_rotated_vertices: (+w, +h), (+w, -h), (-w, -h), (-w, +h) halves."""
    ax, ay = _axes(b[:, 4])
    hw, hh = 0.5 * b[:, 2:3], 0.5 * b[:, 3:4]
    c = b[:, :2]
    return torch.stack([c + hw * ax + hh * ay, c + hw * ax - hh * ay, c - hw * ax - hh * ay, c - hw * ax + hh * ay], 1)


def _clip(poly, cnt, axis, sign, bound):
    """One Sutherland-Hodgman pass: keep ``sign * x[axis] <= bound``.  poly (P, 8, 2), cnt (P) vertices in use -> the same."""
    P, M, _ = poly.shape
    idx = torch.arange(M)[None]
    valid = idx < cnt[:, None]
    nxt_i = torch.where(idx + 1 < cnt[:, None], idx + 1, torch.zeros_like(idx))
    nxt = torch.gather(poly, 1, nxt_i[..., None].expand(-1, -1, 2))
    d0 = bound[:, None] - sign * poly[..., axis]
    d1 = bound[:, None] - sign * nxt[..., axis]
    in0, in1 = d0 >= 0, d1 >= 0
    emit_v, emit_x = valid & in0, valid & (in0 != in1)
    t = d0 / torch.where(emit_x, d0 - d1, torch.ones_like(d0))
    cross = poly + t[..., None] * (nxt - poly)
    n_emit = emit_v.long() + emit_x.long()
    start = torch.cumsum(n_emit, 1) - n_emit
    dump = torch.full_like(start, M)                                  # slot M collects what is not emitted and is cut off below
    pos_v = torch.where(emit_v, start, dump)
    pos_x = torch.where(emit_x, start + emit_v.long(), dump)
    out = torch.zeros((P, M + 1, 2), dtype=poly.dtype)
    out = out.scatter(1, pos_v[..., None].expand(-1, -1, 2), poly)
    out = out.scatter(1, pos_x[..., None].expand(-1, -1, 2), cross)
    new_cnt = n_emit.sum(1)
    assert int(new_cnt.max()) <= M
    return out[:, :M], new_cnt


def intersection_area(a, b):
    va = vertices(a) - b[:, None, :2]
    bx, by = _axes(b[:, 4])
    local = torch.stack([(va * bx[:, None]).sum(-1), (va * by[:, None]).sum(-1)], -1)          # a's vertices in b's frame
    poly = torch.cat([local, torch.zeros_like(local)], 1)
    cnt = torch.full((a.shape[0],), 4, dtype=torch.int64)
    for axis, half in ((0, 0.5 * b[:, 2]), (1, 0.5 * b[:, 3])):
        for sign in (1.0, -1.0):
            poly, cnt = _clip(poly, cnt, axis, sign, half)
    idx = torch.arange(8)[None]
    valid = idx < cnt[:, None]
    nxt_i = torch.where(idx + 1 < cnt[:, None], idx + 1, torch.zeros_like(idx))
    nxt = torch.gather(poly, 1, nxt_i[..., None].expand(-1, -1, 2))
    cr = poly[..., 0] * nxt[..., 1] - poly[..., 1] * nxt[..., 0]
    return 0.5 * torch.where(valid, cr, torch.zeros_like(cr)).sum(1).abs()


def iou(a, b):
    """(P, 5), (P, 5) float64 -> (P) IoU of the pairs (a[i], b[i]); differentiable in both."""
    assert a.dtype == F64 and b.dtype == F64
    inter = intersection_area(a, b)
    return inter / (a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3] - inter)


def loss_and_grad(a, b):
    """-> (1 - IoU (P), d sum(1 - IoU) / d a (P, 5)), float64 autograd."""
    ar = a.detach().clone().requires_grad_(True)
    l = 1.0 - iou(ar, b)
    (g,) = torch.autograd.grad(l.sum(), ar)
    return l.detach(), g


def _seg_dist(p, s0, s1):
    """points p (P, 4, 1, 2) to segments s0 -> s1 (P, 1, 4, 2) -> (P, 4, 4)."""
    d = s1 - s0
    t = (((p - s0) * d).sum(-1) / (d * d).sum(-1).clamp_min(1e-300)).clamp(0.0, 1.0)
    return (p - (s0 + t[..., None] * d)).norm(dim=-1)


def margin(a, b):
    va, vb = vertices(a.detach()), vertices(b.detach())
    da = _seg_dist(va[:, :, None], vb[:, None], vb.roll(-1, 1)[:, None])
    db = _seg_dist(vb[:, :, None], va[:, None], va.roll(-1, 1)[:, None])
    return torch.minimum(da.flatten(1).min(1).values, db.flatten(1).min(1).values)


def generate(count, seed):
    """-> (pred, gt) float64 (count, 5): gt cx, cy ~ U(16, 112), w ~ U(8, 96), h ~ U(2, 16), angle ~ U(-180, 180); the prediction is the
    gt plus N(0, 3) on the centre, N(0, 6) on w, N(0, 2) on h, N(0, 15) degrees on the angle; w and h floored at 1."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(count, generator=g, dtype=F64)
    n = lambda s: s * torch.randn(count, generator=g, dtype=F64)
    gt = torch.stack([u(16, 112), u(16, 112), u(8, 96), u(2, 16), u(-180, 180)], 1)
    pred = gt + torch.stack([n(3), n(3), n(6), n(2), n(15)], 1)
    pred[:, 2:4] = pred[:, 2:4].clamp_min(1.0)
    return pred, gt


def special_cases():
    """-> (pred (S, 5), gt (S, 5), forward_only (S) bool, names).  Everything not forward_only is at least 0.05 px away from a kink."""
    rows = [
        ("parallel", [50.0, 40.0, 30.0, 8.0, 25.0], [52.0, 41.5, 34.0, 10.0, 25.0], False),          # equal angles, no collinear edges
        ("pred_inside_gt", [60.0, 60.0, 10.0, 3.0, 12.0], [61.0, 60.5, 40.0, 12.0, 20.0], False),
        ("gt_inside_pred", [61.0, 60.5, 40.0, 12.0, 20.0], [60.0, 60.0, 10.0, 3.0, 12.0], False),
        ("disjoint", [20.0, 20.0, 10.0, 4.0, 30.0], [90.0, 100.0, 12.0, 5.0, -40.0], False),
        ("swapped_90", [40.0, 50.0, 24.0, 6.0, 10.0], [40.0, 50.0, 6.0, 24.0, 100.0], True),         # the same rectangle described twice
        ("swapped_90_moved", [41.0, 50.5, 24.0, 6.0, 10.0], [40.0, 50.0, 7.0, 26.0, 100.0], False),
        ("plus_minus_180", [70.0, 30.0, 20.0, 5.0, 180.0], [71.5, 30.6, 22.0, 6.0, -180.0], False),
        ("across_the_wrap", [70.0, 30.0, 20.0, 5.0, 179.9], [70.8, 31.0, 23.0, 6.0, -179.9], False),
        ("one_to_fifty", [64.0, 64.0, 100.0, 2.0, 33.0], [64.5, 64.3, 96.0, 2.4, 34.0], False),
        ("identical", [33.0, 44.0, 28.0, 7.0, -17.0], [33.0, 44.0, 28.0, 7.0, -17.0], True),
    ]
    pred = torch.tensor([r[1] for r in rows], dtype=F64)
    gt = torch.tensor([r[2] for r in rows], dtype=F64)
    return pred, gt, torch.tensor([r[3] for r in rows]), [r[0] for r in rows]


def decode(deltas, anchors, weights, clamp=math.log(1000.0 / 16)):
    """Box2BoxTransformRotated.apply_deltas without the angle wrap's jump mattering to the IoU (the wrapped angle describes the same box):
    deltas, anchors (P, 5) -> boxes (P, 5); differentiable in the deltas."""
    wx, wy, ww, wh, wa = weights
    dw, dh = (deltas[:, 2] / ww).clamp(max=clamp), (deltas[:, 3] / wh).clamp(max=clamp)
    ang = deltas[:, 4] / wa * 180.0 / math.pi + anchors[:, 4]
    ang = (ang + 180.0) % 360.0 - 180.0
    return torch.stack([deltas[:, 0] / wx * anchors[:, 2] + anchors[:, 0], deltas[:, 1] / wy * anchors[:, 3] + anchors[:, 1],
                        torch.exp(dw) * anchors[:, 2], torch.exp(dh) * anchors[:, 3], ang], 1)
