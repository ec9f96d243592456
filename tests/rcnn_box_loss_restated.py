"""The R-CNN heads' IoU box losses (BBOX_REG_LOSS_TYPE "giou", "rotated_iou", "rotated_giou") restated in float64 torch for the tests of
sod_rows_box_loss_*, FastRCNNOutputLayers and RPN / RRPN: a helper, not reference code.  The rotated IoU, the rotated decode and the
exclusion mask are those of tests/rotated_iou_loss_restated.py (RL) and tests/rotated_giou_loss_restated.py (GL).

  giou_xyxy(b1, b2)        fvcore's giou_loss of XYXY pairs, eps 1e-7, per pair.
  decode_xyxy(d, b, w)     Box2BoxTransform.apply_deltas (dw, dh clamped at log(1000 / 16)); differentiable in the deltas.
  get_deltas_rotated       Box2BoxTransformRotated.get_deltas / Box2BoxTransform.get_deltas in float64 (the tests' inputs come from them).
  / get_deltas_xyxy
  row_deltas(...)          the D columns a row's loss reads: Fast R-CNN rows (foreground 0 <= label < K, columns label * D ...) or RPN rows
                           (foreground label == 1, columns 0 ... D).
  rows_loss(...)           detectron2's box_reg_loss before its normaliser: the sum over the foreground rows of
                           loss(apply_deltas(fg deltas, src), gt); with autograd, its gradient w.r.t. the whole (R, ld) prediction.
  rotated_rows(n, m)       the input recipe of the rotated-row tests (see there).
"""
import math

import torch

import rotated_giou_loss_restated as GL
import rotated_iou_loss_restated as RL

F64 = torch.float64
SCALE_CLAMP = math.log(1000.0 / 16)
DIMS = {"giou": 4, "rotated_iou": 5, "rotated_giou": 5}


def giou_xyxy(b1, b2, eps=1e-7):
    x1, y1, x2, y2 = b1.unbind(-1)
    x1g, y1g, x2g, y2g = b2.unbind(-1)
    xk1, yk1, xk2, yk2 = torch.max(x1, x1g), torch.max(y1, y1g), torch.min(x2, x2g), torch.min(y2, y2g)
    overlap = (xk2 > xk1) & (yk2 > yk1)
    inter = torch.where(overlap, (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(x1))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    iou = inter / (union + eps)
    area_c = (torch.max(x2, x2g) - torch.min(x1, x1g)) * (torch.max(y2, y2g) - torch.min(y1, y1g))
    return 1.0 - (iou - (area_c - union) / (area_c + eps))


def decode_xyxy(deltas, boxes, weights, clamp=SCALE_CLAMP):
    wx, wy, ww, wh = weights
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    dw, dh = (deltas[:, 2] / ww).clamp(max=clamp), (deltas[:, 3] / wh).clamp(max=clamp)
    pcx, pcy = deltas[:, 0] / wx * w + cx, deltas[:, 1] / wy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)


def get_deltas_xyxy(src, tgt, weights):
    wx, wy, ww, wh = weights
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    return torch.stack([wx * (tgt[:, 0] + 0.5 * tw - src[:, 0] - 0.5 * sw) / sw, wy * (tgt[:, 1] + 0.5 * th - src[:, 1] - 0.5 * sh) / sh,
                        ww * torch.log(tw / sw), wh * torch.log(th / sh)], 1)


def get_deltas_rotated(src, tgt, weights):
    wx, wy, ww, wh, wa = weights
    da = (tgt[:, 4] - src[:, 4] + 180.0) % 360.0 - 180.0
    return torch.stack([wx * (tgt[:, 0] - src[:, 0]) / src[:, 2], wy * (tgt[:, 1] - src[:, 1]) / src[:, 3], ww * torch.log(tgt[:, 2] / src[:, 2]),
                        wh * torch.log(tgt[:, 3] / src[:, 3]), wa * da * math.pi / 180.0], 1)


def foreground(rows, labels, K):
    labels = labels.long()
    return (labels == 1) if rows == "rpn" else ((labels >= 0) & (labels < K))


def row_deltas(rows, pred, labels, K, D):
    """pred (R, ld), labels (R) -> (foreground mask (R), the foreground rows' deltas (F, D), their first columns (F))."""
    fg = foreground(rows, labels, K)
    c0 = torch.zeros(int(fg.sum()), dtype=torch.long) if rows == "rpn" else labels.long()[fg] * D
    cols = c0[:, None] + torch.arange(D)[None]
    return fg, torch.gather(pred[fg], 1, cols), c0


def decode(kind, deltas, src, weights):
    return decode_xyxy(deltas, src, weights) if kind == "giou" else RL.decode(deltas, src, weights)


def pair_loss(kind, boxes, gt):
    if kind == "giou":
        return giou_xyxy(boxes, gt)
    return 1.0 - RL.iou(boxes, gt) if kind == "rotated_iou" else GL.loss(boxes, gt)


def rows_loss(kind, rows, pred, labels, K, src, gt, weights):
    """float64 throughout -> (sum over the foreground rows (python float), d sum / d pred (R, ld), foreground mask, decoded boxes (F, D))."""
    D = DIMS[kind]
    p = pred.double().detach().clone().requires_grad_(True)
    fg, d, _ = row_deltas(rows, p, labels, K, D)
    boxes = decode(kind, d, src.double()[fg], weights)
    total = pair_loss(kind, boxes, gt.double()[fg]).sum()
    if total.requires_grad:
        (g,) = torch.autograd.grad(total, p)
    else:                                                  # no foreground row
        g = torch.zeros_like(p)
    return float(total.detach()), g, fg, boxes.detach()


# ------------------------------------------------------------------------------------------------ the rotated-row recipe
W_ROI5 = (10.0, 10.0, 5.0, 5.0, 1.0)


def rotated_rows(near=192, far=192, K=3, seed=17):
    """The rotated rows of the GPU test, as Fast R-CNN rows: wanted boxes and gts = RL.generate(near, 11) + GL.generate_far(far, 13);
    proposals = the wanted box jittered (generator ``seed``: centre +- 10 % of its own w, h; sizes x exp(+- 0.2); angle +- 10 degrees);
    deltas = get_deltas(proposal, wanted) in float64, so a row decodes to its wanted box up to float32 rounding.  Everything is rounded
    to float32 (what the kernel sees) and returned as float32.  K classes, ld = ceil8(K * 5); the foreground class cycles 0 .. K - 1,
    every 7th row is background (label K); the other classes' columns and the pad columns hold large finite random numbers.
    -> pred (R, ld), labels (R) int32, src (R, 5), gt (R, 5)."""
    pn, gn = RL.generate(near, 11)
    pf, gf = GL.generate_far(far, 13)
    wanted, gt = torch.cat([pn, pf]).float().double(), torch.cat([gn, gf]).float().double()
    R = wanted.shape[0]
    g = torch.Generator().manual_seed(seed)
    r_c, r_s, r_a = torch.rand(R, 2, generator=g, dtype=F64), torch.rand(R, 2, generator=g, dtype=F64), torch.rand(R, generator=g, dtype=F64)
    src = torch.cat([wanted[:, :2] + (r_c - 0.5) * 0.2 * wanted[:, 2:4], wanted[:, 2:4] * torch.exp((r_s - 0.5) * 0.4),
                     (wanted[:, 4] + (r_a - 0.5) * 20.0)[:, None]], 1).float().double()
    deltas = get_deltas_rotated(src, wanted, W_ROI5).float()
    ld = (K * 5 + 7) // 8 * 8
    labels = (torch.arange(R) % K).to(torch.int32)
    labels[6::7] = K
    pred = (torch.randn(R, ld, generator=g, dtype=F64) * 1e3).float()
    fg = labels < K
    cols = labels.long()[fg, None] * 5 + torch.arange(5)[None]
    pred[fg] = pred[fg].scatter(1, cols, deltas[fg])
    return pred, labels, src.float(), gt.float()
