"""The Gaussian KL-divergence box loss restated in float64 torch for the tests of layers.rotated_kld_loss, sod_rotated_kld_loss,
sod_retina_rkld_loss_* and the "rotated_kld" kind of sod_rows_box_loss_*: a helper, not reference code, and the arbiter of those tests.
It is built from the covariance MATRICES (R diag R^T, torch.linalg.inv, logdet, log1p) - not from the closed form the kernel evaluates
(csrc/gauss_box_loss.h); tests/test_rotated_kld_loss_host.py holds the closed form against it.

  gaussian(b)          boxes (P, 5) = (cx, cy, w, h, angle_deg), detectron2's axes (width along (cos t, -sin t), height along (sin t, cos t))
                       -> mean (P, 2), covariance (P, 2, 2) = R diag(w^2 / 4, h^2 / 4) R^T, the columns of R being the two axes.
  kld(a, b)            KL(N_a || N_b) = 1/2 d^T Sb^-1 d + 1/2 Tr(Sb^-1 Sa) + 1/2 (logdet Sb - logdet Sa) - 1.
  loss(a, b)           1 - 1 / (1 + log1p(kld)), tau = 1.
  loss_and_grad(a, b)  -> (loss (P), d sum(loss) / d a (P, 5)), float64 autograd; the angle's column per degree.
  restated_sum(...)    the decode-and-sum over the positives of a RetinaNet buffer (the helper of tests/test_gpu_rotated_giou_loss.py).
  rows_loss(...)       the same over Fast R-CNN / RPN rows (tests/rcnn_box_loss_restated.py's rows_loss for this loss).
  lift(x)              rounds to float32 (what the kernel sees), then lifts to float64.
  row_errors(...)      worst |L - L64| and worst gradient-row error over its row norm.  The norm has no floor, as in
                       tests/test_gpu_rotated_giou_loss.py: a row is divided by its own float64 norm.  That file compares no row whose
                       exact gradient is zero (identical boxes are forward-only there); here such rows ARE compared - a float64 norm
                       below ZERO_NORM = 1e-9 is the rounding of an exact zero - and count by their absolute error, "within the bar of 0".
One pair is beyond float64 matrices: the sliver of special_cases() (condition number of the gt's covariance 2.8e17; inv / logdet give
0.9718).  Its arbiter is SLIVER_LOSS, the matrix definition at 50 digits (tests/test_rotated_kld_loss_host.py computes it).
The pair generators are RL.generate and GL.generate_far; RL.decode is the rotated apply_deltas.
"""
import math

import torch

import rcnn_box_loss_restated as RR
import rotated_giou_loss_restated as GL
import rotated_iou_loss_restated as RL

F64 = torch.float64
RATIOS = (1, 2, 5, 10, 50)
ZERO_NORM = 1e-9
# gt (100, 100, 8000, 1.5e-5, 10) against prediction (101, 100, 7000, 1, 12): the sliver an undamped random-init R-CNN decoded to
SLIVER_PRED, SLIVER_GT, SLIVER_LOSS = [101.0, 100.0, 7000.0, 1.0, 12.0], [100.0, 100.0, 8000.0, 1.5e-5, 10.0], 0.97016578


def lift(x):
    return x.float().double()


def gaussian(b):
    assert b.dtype == F64
    t = b[:, 4] * (math.pi / 180.0)
    c, s = torch.cos(t), torch.sin(t)
    rot = torch.stack([torch.stack([c, s], -1), torch.stack([-s, c], -1)], -2)          # rows (c, s), (-s, c): columns ax = (c, -s), ay = (s, c)
    diag = torch.diag_embed(torch.stack([b[:, 2] ** 2 / 4.0, b[:, 3] ** 2 / 4.0], -1))
    return b[:, :2], rot @ diag @ rot.transpose(-1, -2)


def kld(a, b):
    ma, sa = gaussian(a)
    mb, sb = gaussian(b)
    inv = torch.linalg.inv(sb)
    d = (ma - mb)[..., None]
    maha = (d.transpose(-1, -2) @ inv @ d)[:, 0, 0]
    trace = (inv @ sa).diagonal(dim1=-2, dim2=-1).sum(-1)
    return 0.5 * maha + 0.5 * trace + 0.5 * (torch.logdet(sb) - torch.logdet(sa)) - 1.0


def loss(a, b):
    assert a.dtype == F64 and b.dtype == F64
    return 1.0 - 1.0 / (1.0 + torch.log1p(kld(a, b)))


def loss_and_grad(a, b):
    ar = a.detach().clone().requires_grad_(True)
    l = loss(ar, b)
    (g,) = torch.autograd.grad(l.sum(), ar)
    return l.detach(), g


def restated_sum(pdel, anchors, matched, pos, weights):
    """sum over the positives of loss(decode(deltas, anchor), matched gt) in float64 and its gradient w.r.t. the deltas (N, R, 5)."""
    N, R = pos.shape
    pd = pdel.double().clone().requires_grad_(True)
    anc = anchors.double()[None].expand(N, -1, -1)
    boxes = RL.decode(pd[pos], anc[pos], weights)
    total = loss(boxes, matched.double()[pos]).sum()
    (g,) = torch.autograd.grad(total, pd)
    return float(total.detach()), g, boxes.detach()


def rows_loss(rows, pred, labels, K, src, gt, weights):
    """float64 -> (sum over the foreground rows (python float), d sum / d pred (R, ld), foreground mask, decoded boxes (F, 5))."""
    p = pred.double().detach().clone().requires_grad_(True)
    fg, d, _ = RR.row_deltas(rows, p, labels, K, 5)
    boxes = RL.decode(d, src.double()[fg], weights)
    total = loss(boxes, gt.double()[fg]).sum()
    if total.requires_grad:
        (g,) = torch.autograd.grad(total, p)
    else:                                                  # no foreground row
        g = torch.zeros_like(p)
    return float(total.detach()), g, fg, boxes.detach()


def pairs(near, far, near_seed=5, far_seed=7):
    """RL.generate(near) + GL.generate_far(far), lifted from float32; every side is positive (asserted)."""
    pn, gn = RL.generate(near, near_seed)
    pf, gf = GL.generate_far(far, far_seed)
    pred, gt = lift(torch.cat([pn, pf])), lift(torch.cat([gn, gf]))
    assert float(pred[:, 2:4].min()) > 0 and float(gt[:, 2:4].min()) > 0
    return pred, gt


def slender(ratio, long_side=100.0, err_deg=3.0):
    """Equal centres and sizes, ``err_deg`` of angle error, a ``long_side`` x ``long_side / ratio`` box -> (pred (1, 5), gt (1, 5))."""
    gt = torch.tensor([[60.0, 50.0, long_side, long_side / ratio, 20.0]], dtype=F64)
    pred = gt.clone()
    pred[0, 4] += err_deg
    return lift(pred), lift(gt)


def special_cases():
    """-> (pred (S, 5), gt (S, 5), names): identical boxes, one box written three ways, squares at 0 and 45 degrees of angle error, the
    five slenderness ratios, the sliver pair."""
    box = [33.0, 44.0, 28.0, 7.0, -17.0]
    rows = [("identical", box, box), ("swapped_90", [33.0, 44.0, 7.0, 28.0, 73.0], box), ("plus_180", [33.0, 44.0, 28.0, 7.0, 163.0], box),
            ("minus_180", [33.0, 44.0, 28.0, 7.0, -197.0], box), ("square_0", [50.0, 40.0, 24.0, 24.0, 0.0], [50.0, 40.0, 24.0, 24.0, 0.0]),
            ("square_45", [50.0, 40.0, 24.0, 24.0, 45.0], [50.0, 40.0, 24.0, 24.0, 0.0])]
    pred = torch.tensor([r[1] for r in rows], dtype=F64)
    gt = torch.tensor([r[2] for r in rows], dtype=F64)
    names = [r[0] for r in rows]
    for ratio in RATIOS:
        p, g = slender(ratio)
        pred, gt = torch.cat([pred, p]), torch.cat([gt, g])
        names.append(f"ratio_{ratio}")
    pred = torch.cat([pred, torch.tensor([SLIVER_PRED], dtype=F64)])
    gt = torch.cat([gt, torch.tensor([SLIVER_GT], dtype=F64)])
    return lift(pred), lift(gt), names + ["sliver"]


def row_errors(got_l, got_g, ref_l, ref_g):
    """-> (worst |L - L64|, worst gradient-row error over the row's float64 norm - a row whose float64 norm is below ZERO_NORM counting by
    its absolute error -, all rows together |e| / |ref|)."""
    e = got_g.double() - ref_g
    n = ref_g.norm(dim=1)
    row = e.norm(dim=1) / torch.where(n > ZERO_NORM, n, torch.ones_like(n))
    err_l = float((got_l.double() - ref_l).abs().max()) if got_l is not None else 0.0
    return err_l, float(row.max()), float(e.norm() / ref_g.norm().clamp_min(1e-300))
