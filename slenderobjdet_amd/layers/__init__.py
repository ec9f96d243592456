"""Operator layer: thin Python over the C-ABI HIP kernels (replaces ``slender_det/layers`` for the hot path)."""


def __getattr__(name):
    # ``from slenderobjdet_amd.layers import rotated_iou_loss`` without importing the loss module together with the package: what a
    # program loads when it imports a sub-module of ``layers`` stays what it was
    if name in ("rotated_iou_loss", "rotated_giou_loss", "rotated_kld_loss"):
        from . import losses

        return getattr(losses, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
