"""Loss operators with the reference's signatures, running on the HIP kernels (autograd-enabled).

  sigmoid_focal_loss(_jit)  — fvcore.nn.sigmoid_focal_loss_jit as called at slender_det/modeling/meta_arch/fcos/fcosv2.py:124
  iou_loss                  — slender_det/layers/iou_loss.py:4-37
  rotated_iou_loss          — 1 - IoU of rotated box pairs (no counterpart in the reference), csrc/rotated_iou_loss.hip
  rotated_giou_loss         — the same with the convex-hull term of GIoU, which keeps a gradient for pairs that do not overlap
  rotated_kld_loss          — the Kullback-Leibler divergence of the boxes' Gaussians (Yang et al., NeurIPS 2021), csrc/gauss_box_loss.h
The three rotated ones are pair operators: one kernel skeleton (csrc/pair_loss.h) and one op-layer helper (functional._pair_loss), which
they share with giou_loss_xyxy and smooth_l1_loss of layers.functional.
"""
import torch
from torch.autograd.function import once_differentiable

from . import functional as HF


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, alpha, gamma, reduction):
        x = inputs.contiguous().float()
        shape = x.shape
        x2 = x.view(-1, shape[-1])
        if targets.dtype in (torch.int32, torch.int64) and targets.dim() == inputs.dim() - 1:
            labels, dense = targets.reshape(-1).to(torch.int32).contiguous(), None
        else:
            labels, dense = None, targets.contiguous().float().view(-1, shape[-1])
        s, elem = HF.focal_loss_fwd(x2, labels, dense, alpha, gamma, want_elem=(reduction == "none"))
        ctx.save_for_backward(x2, labels if labels is not None else dense)
        ctx.cfg = (alpha, gamma, reduction, labels is not None, shape)
        if reduction == "none":
            return elem.view(shape)
        return s[0] / x2.numel() if reduction == "mean" else s[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x2, t = ctx.saved_tensors
        alpha, gamma, reduction, is_labels, shape = ctx.cfg
        labels, dense = (t, None) if is_labels else (None, t)
        if reduction == "none":
            grad = HF.focal_loss_bwd(x2, labels, dense, alpha, gamma).view(shape) * g
        else:
            scale = g.reshape(1).float().contiguous()
            if reduction == "mean":
                scale = scale / x2.numel()
            grad = HF.focal_loss_bwd(x2, labels, dense, alpha, gamma, scale_num=scale).view(shape)
        return grad, None, None, None, None


def sigmoid_focal_loss(inputs, targets, alpha: float = -1, gamma: float = 2, reduction: str = "none"):
    """``targets``: float one-hot/soft tensor like ``inputs`` (the fvcore contract) or integer class indices of shape
    ``inputs.shape[:-1]`` (value outside [0, K) = background; avoids materialising the one-hot)."""
    return _FocalFn.apply(inputs, targets, float(alpha), float(gamma), reduction)


sigmoid_focal_loss_jit = sigmoid_focal_loss


class _IouLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, loss_type):
        p, t = pred.contiguous().float(), target.contiguous().float()
        w = weight.contiguous().float() if weight is not None else None
        s, _ = HF.iou_loss_fwd(p, t, w, loss_type)
        ctx.save_for_backward(p, t, w)
        ctx.loss_type = loss_type
        return s[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, t, w = ctx.saved_tensors
        return HF.iou_loss_bwd(p, t, w, ctx.loss_type, grad_scale=g.reshape(1).float().contiguous()), None, None, None


def iou_loss(pred, target, weight=None, loss_type="iou"):
    """Weighted SUM of the per-row IoU / linear-IoU / GIoU loss on (l, t, r, b) distances."""
    if loss_type not in HF.IOU_TYPES:
        raise NotImplementedError(loss_type)
    if weight is None:
        assert pred.shape[0] != 0
    return _IouLossFn.apply(pred, target, weight, loss_type)


class _BceSoftFn(torch.autograd.Function):
    """F.binary_cross_entropy_with_logits(x[fg], t[fg], reduction="sum") with fg = rows whose label is a foreground class; the rows
    are selected by the label inside the kernel (no boolean gather)."""

    @staticmethod
    def forward(ctx, logits, targets, labels, bg_label):
        x, t, l = logits.contiguous().float(), targets.contiguous().float(), labels.contiguous().to(torch.int32)
        ctx.save_for_backward(x, t, l)
        ctx.bg = int(bg_label)
        return HF.bce_logits_soft_fwd(x, t, l, ctx.bg)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, t, l = ctx.saved_tensors
        return HF.bce_logits_soft_bwd(x, t, l, ctx.bg, g.reshape(1).float().contiguous()), None, None, None


def bce_with_logits_fg_sum(logits, targets, labels, bg_label):
    return _BceSoftFn.apply(logits, targets, labels, bg_label)


class _RotatedIouLossFn(torch.autograd.Function):
    """``ops``: the (fwd, bwd) pair of the op layer - rotated IoU, rotated GIoU or the Gaussian KL divergence."""

    @staticmethod
    def forward(ctx, pred, target, reduction, ops):
        p, t = pred.contiguous().float(), target.contiguous().float()
        elem, s = ops[0](p, t, want_elem=(reduction == "none"))
        ctx.save_for_backward(p, t)
        ctx.reduction, ctx.bwd = reduction, ops[1]
        if reduction == "none":
            return elem.view(pred.shape[:-1])
        return s[0] / max(p.shape[0], 1) if reduction == "mean" else s[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        if ctx.reduction == "none":
            return ctx.bwd(p, t) * g.reshape(-1, 1).float(), None, None, None
        scale = g.reshape(1).float().contiguous()
        if ctx.reduction == "mean":
            scale = scale / max(p.shape[0], 1)
        return ctx.bwd(p, t, grad_scale=scale), None, None, None


def _rotated_pair_loss(name, ops, pred, target, reduction):
    if reduction not in ("sum", "mean", "none"):
        raise ValueError(f"{name}: reduction must be 'sum', 'mean' or 'none', got {reduction!r}")
    if pred.dim() != 2 or pred.shape[-1] != 5 or pred.shape != target.shape:
        raise ValueError(f"{name}: pred and target must both be (P, 5), got {tuple(pred.shape)} and {tuple(target.shape)}")
    return _RotatedIouLossFn.apply(pred, target, reduction, ops)


def rotated_iou_loss(pred, target, reduction="sum"):
    """1 - IoU(pred, target) of (P, 5) rotated boxes (cx, cy, w, h, angle_deg), the IoU being box_iou_rotated's (detectron2's); the
    gradient flows to ``pred`` only, its angle column per degree.  Boxes that do not overlap (IoU exactly 0) have loss 1 and NO gradient:
    use it on matched pairs (a positive anchor and its gt), not to pull distant boxes together.  The IoU has kinks where a vertex of one
    box lies on an edge of the other and at identical boxes; the gradient there is the one of a side.  rotated_giou_loss is the loss
    that keeps a gradient for boxes that do not overlap."""
    return _rotated_pair_loss("rotated_iou_loss", (HF.rotated_iou_loss_fwd, HF.rotated_iou_loss_bwd), pred, target, reduction)


def rotated_giou_loss(pred, target, reduction="sum"):
    """1 - IoU + (C - U) / C of (P, 5) rotated boxes (cx, cy, w, h, angle_deg) in [0, 2): the IoU of rotated_iou_loss (to the bit), U the
    union and C the area of the convex hull of the 8 corners.  The gradient flows to ``pred`` only, its angle column per degree; boxes
    that do not overlap have loss 1 + (C - U) / C and the hull term's gradient, which pulls them together.  Besides the kinks of the
    IoU the loss has kinks where a corner enters or leaves the hull (collinear or coincident corners: identical boxes, equal angles
    with a shared edge line); the value is right there and the gradient is the one of a side (csrc/box_pair_loss.h says which)."""
    return _rotated_pair_loss("rotated_giou_loss", (HF.rotated_giou_loss_fwd, HF.rotated_giou_loss_bwd), pred, target, reduction)


def rotated_kld_loss(pred, target, reduction="sum"):
    """The Gaussian KL-divergence loss of (P, 5) rotated boxes (cx, cy, w, h, angle_deg) (Yang et al., NeurIPS 2021).  A box is the
    Gaussian N(mu, S) with mu = (cx, cy) and S = R diag(w^2 / 4, h^2 / 4) R^T, R turning the width axis to (cos t, -sin t); then

        D = KL(N_pred || N_target) = 1/2 (mu_p - mu_t)^T S_t^-1 (mu_p - mu_t) + 1/2 Tr(S_t^-1 S_p) + 1/2 ln(|S_t| / |S_p|) - 1
        loss = 1 - 1 / (1 + ln(1 + D))            in [0, 1), 0 exactly when the two Gaussians coincide.

    The gradient flows to ``pred`` only, its angle column per degree.  The loss is smooth wherever the sides are positive (no kinks:
    nothing is clipped), keeps a gradient for boxes that do not overlap, and its angle gradient grows with the squared aspect ratio.
    Invariances: it depends on the Gaussian, not on how the box is written - (w, h, t), (h, w, t + 90) and t +- 180 give the same value.
    Limits: a SQUARE box is an isotropic Gaussian, so its angle has no effect on the loss and gets gradient 0 (if either box is square
    the angle column is exactly 0) - the loss cannot orient a square; a side of either box that is not positive or not finite gives NaN,
    value and gradient."""
    return _rotated_pair_loss("rotated_kld_loss", (HF.rotated_kld_loss_fwd, HF.rotated_kld_loss_bwd), pred, target, reduction)
