"""The rotated GIoU loss restated in float64 torch for the tests of layers.rotated_giou_loss, sod_rotated_giou_loss and
sod_retina_rgiou_loss_*: a helper, not reference code.  The IoU, the vertices, the pair generator and the decode are those of
tests/rotated_iou_loss_restated.py (RL).

  hull_area(a, b)     area of the convex hull of the 8 corners.  The hull's vertex indices come from the DETACHED corners (Andrew's
                      monotone chain, a Python loop per pair, collinear points dropped); the shoelace sum runs over the gathered, still
                      differentiable corners, so autograd gives d C / d a - by another route than the kernel's walk over sorted points.
  loss(a, b)          1 - IoU + (C - U) / C with U = area(a) + area(b) - I.
  hull_margin(a, b)   the minimum over the 8 corners of the distance from that corner to the boundary of the convex hull of the other 7:
                      the hull's structure changes exactly where this is 0, and the loss has a kink there.
  excluded(a, b)      hull_margin < 1e-2 px, or RL.margin < 1e-2 px where the boxes overlap (the IoU's own kinks).
  generate_far(n, s)  RL.generate with the prediction's centre moved by N(0, 40) px instead of N(0, 3): most pairs are disjoint.
  special_cases()     RL.special_cases() plus three pairs of this loss's own.
"""
import math

import torch

import rotated_iou_loss_restated as RL

F64 = torch.float64
MARGIN = 1e-2


def corners(a, b):
    """(P, 5), (P, 5) -> (P, 8, 2): the corners of a, then those of b."""
    return torch.cat([RL.vertices(a), RL.vertices(b)], 1)


def _chain(pts):
    """Andrew's monotone chain on 8 (x, y) tuples -> the hull's vertex indices, counter-clockwise, collinear points dropped."""
    order = sorted(range(len(pts)), key=lambda i: pts[i])
    cross = lambda o, p, q: (pts[p][0] - pts[o][0]) * (pts[q][1] - pts[o][1]) - (pts[p][1] - pts[o][1]) * (pts[q][0] - pts[o][0])
    lower, upper = [], []
    for i in order:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], i) <= 0:
            lower.pop()
        lower.append(i)
    for i in reversed(order):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], i) <= 0:
            upper.pop()
        upper.append(i)
    return lower[:-1] + upper[:-1]


def hull_indices(pts):
    """(P, 8, 2) -> (P, 8) int64: each row's hull vertices in order, padded with the last one (a repeated vertex adds no area)."""
    rows = []
    for p in pts.detach().tolist():
        h = _chain([tuple(q) for q in p])
        rows.append(h + [h[-1]] * (8 - len(h)))
    return torch.tensor(rows, dtype=torch.int64).view(-1, 8)


def hull_area(a, b):
    pts = corners(a, b)
    v = torch.gather(pts, 1, hull_indices(pts)[..., None].expand(-1, -1, 2))
    n = v.roll(-1, 1)
    return 0.5 * (v[..., 0] * n[..., 1] - v[..., 1] * n[..., 0]).sum(1)


def hull_term(a, b):
    """(C - U) / C; 0 where C is not positive."""
    inter = RL.intersection_area(a, b)
    union = a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3] - inter
    c = hull_area(a, b)
    safe = torch.where(c > 0, c, torch.ones_like(c))
    return torch.where(c > 0, (c - union) / safe, torch.zeros_like(c))


def hull_term_given_iou(a, b, iou):
    """The hull term as the kernels define it: I and U recovered from a given IoU (the operator's own), I = IoU * asum / (1 + IoU)."""
    asum = a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3]
    union = asum - iou * asum / (1.0 + iou)
    c = hull_area(a, b)
    safe = torch.where(c > 0, c, torch.ones_like(c))
    return torch.where(c > 0, (c - union) / safe, torch.zeros_like(c))


def loss(a, b):
    assert a.dtype == F64 and b.dtype == F64
    return 1.0 - RL.iou(a, b) + hull_term(a, b)


def _grad(fn, a, b):
    ar = a.detach().clone().requires_grad_(True)
    l = fn(ar, b)
    (g,) = torch.autograd.grad(l.sum(), ar)
    return l.detach(), g


def loss_and_grad(a, b):
    """-> (loss (P), d sum(loss) / d a (P, 5)), float64 autograd."""
    return _grad(loss, a, b)


def hull_term_and_grad(a, b):
    return _grad(hull_term, a, b)


def hull_margin(a, b):
    pts = corners(a.detach(), b.detach())                                        # (P, 8, 2)
    P = pts.shape[0]
    p, q, r = pts[:, :, None, None], pts[:, None, :, None], pts[:, None, None, :]
    d = q - p                                                                    # (P, 8, 8, 1, 2)
    side = d[..., 0] * (r - p)[..., 1] - d[..., 1] * (r - p)[..., 0]               # (P, p, q, r): > 0 where r is left of p -> q
    eye = torch.eye(8, dtype=torch.bool)
    seg = (d * d).sum(-1)[..., 0] > 0                                            # (P, p, q): p and q are distinct points
    t = (((r - p) * d).sum(-1) / (d * d).sum(-1).clamp_min(1e-300)).clamp(0.0, 1.0)
    dist = (r - (p + t[..., None] * d)).norm(dim=-1)                             # (P, p, q, r): r to the segment p q
    out = torch.full((P,), float("inf"), dtype=F64)
    for i in range(8):                                                          # the corner left out
        others = torch.ones(8, dtype=torch.bool)
        others[i] = False
        ign = eye[:, None, :] | eye[None, :, :] | ~others[None, None, :]          # (p, q, r): r is p, q or the corner i
        edge = ((side >= -1e-9) | ign[None]).all(-1) & seg & others[None, :, None] & others[None, None, :]
        di = torch.where(edge, dist[..., i], torch.full_like(dist[..., i], float("inf")))
        out = torch.minimum(out, di.flatten(1).min(1).values)
    return out


def excluded(a, b):
    return (hull_margin(a, b) < MARGIN) | ((RL.margin(a, b) < MARGIN) & (RL.iou(a.detach(), b.detach()) > 0))


def generate_far(count, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(count, generator=g, dtype=F64)
    n = lambda s: s * torch.randn(count, generator=g, dtype=F64)
    gt = torch.stack([u(16, 112), u(16, 112), u(8, 96), u(2, 16), u(-180, 180)], 1)
    pred = gt + torch.stack([n(40), n(40), n(6), n(2), n(15)], 1)
    pred[:, 2:4] = pred[:, 2:4].clamp_min(1.0)
    return pred, gt


# shared_edge_line in the prediction's frame (u along the width, v along the height): the prediction is [-15, 15] x [-4, 4], the gt
# [-7, 27] x [-4, 8]: the edges v = -4 lie on one line.  I = 22 * 8, U = 240 + 408 - 176, the hull is the 42 x 12 box without the
# triangle (-15, 4), (-15, 8), (-7, 8).
SHARED_EDGE_LINE_LOSS = 1.0 - 176.0 / 472.0 + (488.0 - 472.0) / 488.0


def special_cases():
    """-> (pred (S, 5), gt (S, 5), forward_only (S) bool, names): RL's, then ``shared_edge_line`` (equal angles of 25 degrees, one
    collinear edge: on a kink of the hull, forward only; the corners are not representable in float32, so the edges are collinear up to
    rounding), ``shared_edge_line_axis`` (the same pair at angle 0, exactly collinear in float32) and ``touching_hull_only`` (disjoint
    boxes a few px apart: only the hull term acts)."""
    pred, gt, fo, names = RL.special_cases()
    t = 25.0 * math.pi / 180.0
    ax, ay = (math.cos(t), -math.sin(t)), (math.sin(t), math.cos(t))
    rows = [
        ("shared_edge_line", [50.0, 40.0, 30.0, 8.0, 25.0], [50.0 + 10.0 * ax[0] + 2.0 * ay[0], 40.0 + 10.0 * ax[1] + 2.0 * ay[1], 34.0, 12.0, 25.0], True),
        ("shared_edge_line_axis", [50.0, 40.0, 30.0, 8.0, 0.0], [60.0, 42.0, 34.0, 12.0, 0.0], True),
        ("touching_hull_only", [40.0, 40.0, 20.0, 6.0, 15.0], [47.0, 52.0, 24.0, 5.0, -30.0], False),
    ]
    pred = torch.cat([pred, torch.tensor([r[1] for r in rows], dtype=F64)])
    gt = torch.cat([gt, torch.tensor([r[2] for r in rows], dtype=F64)])
    return pred, gt, torch.cat([fo, torch.tensor([r[3] for r in rows])]), names + [r[0] for r in rows]
