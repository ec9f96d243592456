"""FCOSRepPoints on the HIP kernels: FCOS stage-1 targets with top-k per box, RepPoints refinement.

Mirror of slender_det/modeling/meta_arch/fcos/fcos_rpd_s1_topk.py:137-746 (``META_ARCHITECTURE: "FCOSRepPoints"``, what
configs/fcos/fcos_reppoints_{R_50,X_152}_FPN_1x.yaml select): same ``cls(cfg)`` constructor contract, same
``forward(batched_inputs)`` contract and loss keys (``cls_loss``, ``reg_loss_init``, ``reg_loss``, ``centerness_loss``).

The model joins two families, and so does this file:
  * the towers are FCOSHead's (multi-level ConvGnRelu launches on two streams, the DCN tower unit included);
  * ``offsets_init`` (9 points per location, fp32 rows pitched 18 -> 24), the DCN offset with its 0.1 gradient multiplier, the two
    DeformConv layers and the ``logits`` / ``offsets_refine`` 1x1 convs are RepPointsDetector's (reppoints.py);
  * stage-1 targets: FCOS assignment, of every gt box only the 5 positives with the largest SLENDER centerness
    ``centerness ** min(w/h, h/w)`` (:25-134), one assignment launch + one selection launch for the batch
    (``sod_fcos_assign_topk_slender``) where the reference loops over images x gts on the host with one ``.item()`` each;
  * boxes are signed LTRB distances taken from the nine points (``offsets2ltrb``, :709-745: ``sod_points2ltrb_*``);
  * stage-2 targets: IoU matcher of every image's gt boxes against ITS predicted init boxes (:343-374), two launches for the batch
    (``sod_fcos_rpd_refine_targets``);
  * the four losses come from the kernels that already compute these formulas (focal, IoU on LTRB with the selection as mask and the
    slender score as weight, stride-normalised smooth-L1, soft-target BCE); their normalisers stay on the device
    (``sod_fcos_rpd_finalize``; the reference reads four of them back, :265-297).
The training step makes no host read.

Kept from the reference, not fixed: the focal term has no valid mask (:279-286: rows outside the image count as background), and
``iou_loss`` sees LTRB values that may be negative, unclamped.  Deviation: with nothing selected the reference divides 0 by 0 in
``reg_loss_init``; here it is 0.  ``MODEL.FCOS.NORM_REG_TARGETS`` is refused (see ``FCOSRepPoints.__init__``).
"""
import math

import torch
import torch.distributed as dist
from torch import nn
from torch.autograd.function import once_differentiable

from ...layers import functional as HF
from ...layers import grad_sched as GS
from ...layers.deform_conv import DeformConv
from ...layers.nn import ConvML, HipConv2d, _arena_of
from ...utils import comm
from .build import META_ARCH_REGISTRY
from .fcos import SIZES_OF_INTEREST, FCOSHead, FCOSV2, _ceil8
from .reppoints import _DcnOffsetFn


class _LevelScaleFn(torch.autograd.Function):
    """``Scale`` l of the head on the fp32 point rows of one level (:639, :660); the scalar is read on the device."""

    @staticmethod
    def forward(ctx, pts, scales, head, level):
        ctx.head, ctx.level = head, level
        ctx.save_for_backward(pts)
        arena = _arena_of(head)
        if arena is not None:
            arena.note_use(head.scales)
        return HF.level_scale_fwd(pts, head.scales.detach()[level:level + 1])

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        head, l = ctx.head, ctx.level
        (pts,) = ctx.saved_tensors
        arena = _arena_of(head)
        dx = HF.level_scale_bwd(dy.contiguous(), pts, head.scales.detach()[l:l + 1], arena.grad_view(head.scales)[l:l + 1])
        arena.mark_ready(head.scales)
        return dx, None, None, None


class FCOSRepPointsHead(FCOSHead):
    """fcos_rpd_s1_topk.py:505-746.  FCOSHead's towers and scales; in place of its two prediction convs the RepPoints part:
    ``offsets_init`` (3x3 + ReLU, 1x1 to 18 padded to 24, fp32), the two DeformConv(relu) layers, ``offsets_refine`` and ``logits``
    (1x1) and a 3x3 ``centerness`` conv padded to 8 output channels."""
    num_points = 9
    gradient_mul = 0.1
    point_strides = (1, 2, 4, 8, 16)        # offsets2ltrb's default argument (:709), NOT the FPN strides

    def __init__(self, cfg, input_shape):
        super().__init__(cfg, input_shape)
        C = self.cls_pred.in_channels
        del self.cls_pred, self.box_pred    # FCOSHead's cls_logits / bbox_pred are commented out in the reference (:614-615)
        self.pts_ld = _ceil8(2 * self.num_points)
        self.k_pad = _ceil8(self.num_classes)
        if len(self.fpn_strides) > len(self.point_strides):
            raise ValueError("FCOSRepPoints: at most five FPN levels (offsets2ltrb has five point strides)")
        self.deform_cls_conv = DeformConv(C, C, 3, 1, 1, relu=True)        # the ReLU that opens ``logits`` / ``offsets_refine`` (:604-613)
        self.deform_reg_conv = DeformConv(C, C, 3, 1, 1, relu=True)
        self.offsets_init = nn.ModuleList([ConvML(C, C, 3, 1, relu=True), ConvML(C, self.pts_ld, 1, 0, out_f32=True)])
        self.offsets_refine = HipConv2d(C, self.pts_ld, 1, 1, 0, bias=True)
        self.logits = HipConv2d(C, self.k_pad, 1, 1, 0, bias=True)
        self.centerness = HipConv2d(C, 8, 3, 1, 1, bias=True)
        npt, K = 2 * self.num_points, self.num_classes
        # :618-639: normal(0.01) / zero bias on the nn.Conv2d instances of the listed modules (DeformConv is none: it keeps its own
        # init); ``logits`` is not listed: its weight keeps torch's default and its bias takes the focal prior
        with torch.no_grad():
            self.offsets_init[0].conv.init_normal(0.01, 0.0)
            self.offsets_init[1].conv.init_normal(0.01, 0.0)
            self.offsets_init[1].conv.weight[npt:].zero_()
            self.offsets_refine.init_normal(0.01, 0.0)
            self.offsets_refine.weight[npt:].zero_()
            self.centerness.init_normal(0.01, 0.0)
            self.centerness.weight[1:].zero_()
            bound = 1.0 / math.sqrt(C)                               # nn.Conv2d default: kaiming_uniform_(a=sqrt(5))
            self.logits.weight.uniform_(-bound, bound)
            self.logits.weight[K:].zero_()
            self.logits.bias.zero_()
            self.logits.bias[:K].fill_(-math.log((1 - cfg.MODEL.FCOS.PRIOR_PROB) / cfg.MODEL.FCOS.PRIOR_PROB))

    def num_logical_params(self):
        """Parameter count of the reference head (the padding rows of the 18 -> 24, K -> k_pad and 1 -> 8 channel convs excluded)."""
        C = self.logits.in_channels
        pad = 2 * (self.pts_ld - 2 * self.num_points) * (C + 1) + (self.k_pad - self.num_classes) * (C + 1) + 7 * (9 * C + 1)
        return sum(p.numel() for p in self.parameters()) - pad

    def run_points(self, cls_t, box_t):
        """:660-698 up to the two DeformConv layers: scaled point rows, relu(dcn(cls tower)), relu(dcn(box tower)) per level."""
        raw = self.offsets_init[1](self.offsets_init[0](list(box_t)))      # per level (N,H,W,24) fp32, x / y interleaved
        oi, cf, rf = [], [], []
        for l in range(len(raw)):
            pts = _LevelScaleFn.apply(raw[l], self.scales, self, l)
            off = _DcnOffsetFn.apply(pts, self.num_points, self.gradient_mul)
            oi.append(pts)
            cf.append(self.deform_cls_conv(cls_t[l], off, off_ld=self.pts_ld))
            rf.append(self.deform_reg_conv(box_t[l], off, off_ld=self.pts_ld))
        return oi, cf, rf

    def predict(self, oi, cf, rf, ctr_in, want_init=True):
        """The three prediction convs and the point transform: logits (N,L,k_pad), centerness (N,L,8; column 0), the refine deltas per
        level, init / refine LTRB (N,L,4) with their arg-point indices, and the decoded init boxes (N,L,4)."""
        for m in (self.logits, self.offsets_refine, self.centerness):
            m.prepare()
        N = cf[0].shape[0]
        hw = [(t.shape[1], t.shape[2]) for t in cf]
        offs, off = [], 0
        for h, w in hw:
            offs.append(off)
            off += h * w
        L, kp, dev = off, self.k_pad, cf[0].device
        logits_buf = torch.empty((N, L, kp), dtype=torch.float32, device=dev)
        HF.conv2d_fwd_ml(list(cf), self.logits.w_bf16, self.logits.bias_eff, 1, 0, 1, out_f32=True,
                         outs=[logits_buf.view(-1)[o * kp:] for o in offs], y_img_stride=L * kp, k_real=self.num_classes)
        ctr_buf = torch.empty((N, L, 8), dtype=torch.float32, device=dev)
        HF.conv2d_fwd_ml(list(ctr_in), self.centerness.w_bf16, self.centerness.bias_eff, 1, 1, 1, out_f32=True,
                         outs=[ctr_buf.view(-1)[o * 8:] for o in offs], y_img_stride=L * 8, k_real=1)
        rdelta = HF.conv2d_fwd_ml(list(rf), self.offsets_refine.w_bf16, self.offsets_refine.bias_eff, 1, 0, 1, out_f32=True)
        refine_ltrb = torch.empty((N, L, 4), dtype=torch.float32, device=dev)
        refine_arg = torch.empty((N, L), dtype=torch.int32, device=dev)
        init_ltrb = init_boxes = init_arg = None
        if want_init:
            init_ltrb = torch.empty((N, L, 4), dtype=torch.float32, device=dev)
            init_boxes = torch.empty((N, L, 4), dtype=torch.float32, device=dev)
            init_arg = torch.empty((N, L), dtype=torch.int32, device=dev)
        for l in range(len(hw)):
            o, s, ps = offs[l], self.fpn_strides[l], self.point_strides[l]
            if want_init:
                HF.points2ltrb_fwd(oi[l], None, s, ps, self.num_points, init_ltrb.view(-1)[o * 4:], init_boxes.view(-1)[o * 4:], L * 4,
                                   init_arg.view(-1)[o:], L)
            # offsets_refine(...) + offsets_init.detach()  (:695-698)
            HF.points2ltrb_fwd(rdelta[l], oi[l], s, ps, self.num_points, refine_ltrb.view(-1)[o * 4:], None, L * 4, refine_arg.view(-1)[o:], L)
        return logits_buf, ctr_buf, rdelta, init_ltrb, init_boxes, init_arg, refine_ltrb, refine_arg, (hw, offs, L)


def rpd_loss_sums(logits_buf, init_ltrb, refine_ltrb, ctr_logit, labels, reg_t, ctr_t, sel32, stats3, cls, cls_bg, refine_t, loc_strides,
                  num_classes, alpha, gamma, iou_loss_type, inv_world, reduce_count=None):
    """FCOSRepPoints.losses (:249-317) on the prediction buffers: -> out8 of ``sod_fcos_rpd_finalize`` (the four losses first) and the
    number of refine positives.  logits_buf (N,L,k_pad), init_ltrb / refine_ltrb (N,L,4), ctr_logit (N,L); stage-1 targets labels /
    reg_t / ctr_t / sel32 (the selection as int32) / stats3 from ``fcos_assign_topk(slender=True)``; stage-2 targets cls / cls_bg /
    refine_t from ``fcos_rpd_refine_targets``; loc_strides (L,) the FPN stride of every location.  ``reduce_count``: the all-reduce of
    the refine count (the stage-1 statistics arrive reduced)."""
    K = num_classes
    focal_sum, _ = HF.focal_loss_fwd(logits_buf, cls_bg, None, alpha, gamma, K=K)      # no valid mask: cls = -1 rows are background
    iou_sum, _ = HF.iou_loss_fwd(init_ltrb.view(-1, 4), reg_t.view(-1, 4), ctr_t.view(-1), iou_loss_type, mask=sel32.view(-1), mask_bg=0)
    sl1 = HF.reppoints_box_loss_fwd(refine_ltrb, refine_t, cls, loc_strides, K, 0.11)   # smooth-L1 of x / (4 * stride), beta 0.11 (:303-307)
    bce_sum = HF.bce_logits_soft_fwd(ctr_logit, ctr_t, labels, K)
    n_refine = sl1[1:2]
    if reduce_count is not None:
        n_refine = n_refine.clone()
        reduce_count(n_refine)
    out8 = HF.fcos_rpd_finalize(focal_sum, iou_sum, sl1, bce_sum, stats3, n_refine, inv_world)
    return out8, n_refine


def rpd_loss_grads(g4, out8, n_refine, logits_buf, init_ltrb, refine_ltrb, ctr_logit, labels, reg_t, ctr_t, sel32, cls, cls_bg, refine_t,
                   loc_strides, num_classes, alpha, gamma, iou_loss_type, inv_world, logits_bf16=False):
    """Gradients of g4 . (the four losses of ``rpd_loss_sums``) with respect to logits_buf (rows of k_pad, bf16 on request), init_ltrb,
    refine_ltrb and ctr_logit.  g4: four one-element fp32 device tensors."""
    K = num_classes
    dlogits = HF.focal_loss_bwd(logits_buf, cls_bg, None, alpha, gamma, K=K, scale_num=g4[0], scale_den=n_refine, den_mul=inv_world, den_min=1.0,
                                ld_out=logits_buf.shape[-1], out_bf16=logits_bf16)
    d_init = HF.iou_loss_bwd(init_ltrb.view(-1, 4), reg_t.view(-1, 4), ctr_t.view(-1), iou_loss_type, mask=sel32.view(-1), mask_bg=0,
                             grad_scale=g4[1] * out8[4:5])
    d_refine = HF.reppoints_box_loss_bwd(refine_ltrb, refine_t, cls, loc_strides, K, 0.11, g4[2] * out8[5:6], out8[7:8], 1.0, 1.0)
    d_ctr = HF.bce_logits_soft_bwd(ctr_logit, ctr_t, labels, K, g4[3] * out8[6:7])
    return dlogits, d_init.view(init_ltrb.shape), d_refine, d_ctr


class _FcosRpdLossFn(torch.autograd.Function):
    """Prediction convs, point transform, refine targets, the four losses and their finalisation (:208-317) as one node over
    (offsets_init, relu(dcn_cls), relu(dcn_reg), centerness tower) of every level."""

    @staticmethod
    def forward(ctx, model, weight, targets, gt, image_hw, inv_world, *tensors):
        head = model.head
        nl = len(tensors) // 4
        oi, cf, rf, ct = (list(tensors[i * nl:(i + 1) * nl]) for i in range(4))
        logits_buf, ctr_buf, rdelta, init_ltrb, init_boxes, init_arg, refine_ltrb, refine_arg, geo = head.predict(oi, cf, rf, ct)
        hw, offs, L = geo
        labels, reg_t, ctr_t, stats3, sel = targets
        boxes, classes, box_off, counts = gt
        K = model.num_classes
        vals, matches, mlab, cls, cls_bg, refine_t = HF.fcos_rpd_refine_targets(
            boxes, classes, box_off, counts, init_boxes, image_hw, hw, head.fpn_strides, K, model.iou_thresholds, model.iou_labels, True)
        ctr_logit = ctr_buf[:, :, 0].contiguous()
        sel32 = sel.to(torch.int32)
        loc_strides = model.loc_strides(hw)
        reduce_count = (lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM)) if comm.collectives_active() else None
        out8, n_refine = rpd_loss_sums(logits_buf, init_ltrb, refine_ltrb, ctr_logit, labels, reg_t, ctr_t, sel32, stats3, cls, cls_bg, refine_t,
                                       loc_strides, K, model.focal_loss_alpha, model.focal_loss_gamma, model.iou_loss_type, inv_world, reduce_count)
        ctx.model, ctx.geo, ctx.nl, ctx.inv_world = model, geo, nl, inv_world
        ctx.save_for_backward(out8, n_refine, logits_buf, init_ltrb, refine_ltrb, ctr_logit, labels, reg_t, ctr_t, sel32, cls, cls_bg, refine_t,
                              loc_strides, init_arg, refine_arg, *cf, *rf, *ct)
        model.last_targets = (labels, reg_t, ctr_t, stats3)
        model.last_refine = (cls, refine_t, matches, mlab, vals)
        arena = _arena_of(head)
        if arena is not None:
            for m in (head.logits, head.offsets_refine, head.centerness):
                arena.note_use(m.weight)
                arena.note_use(m.bias)
        return out8[0], out8[1], out8[2], out8[3]

    @staticmethod
    @once_differentiable
    def backward(ctx, *g4):
        model, (hw, offs, L), nl, inv_world = ctx.model, ctx.geo, ctx.nl, ctx.inv_world
        head = model.head
        (out8, n_refine, logits_buf, init_ltrb, refine_ltrb, ctr_logit, labels, reg_t, ctr_t, sel32, cls, cls_bg, refine_t, loc_strides,
         init_arg, refine_arg) = ctx.saved_tensors[:16]
        rest = ctx.saved_tensors[16:]
        cf, rf, ct = rest[:nl], rest[nl:2 * nl], rest[2 * nl:3 * nl]
        dev = logits_buf.device
        g4 = [g.reshape(1).float() if g is not None else torch.zeros(1, dtype=torch.float32, device=dev) for g in g4]
        N, K, kp, P, ld = logits_buf.shape[0], model.num_classes, head.k_pad, head.num_points, head.pts_ld
        f32 = HF.is_f32()          # validation mode: the gradient rows of offsets_refine (and every other row) stay fp32
        arena = _arena_of(head)
        dlogits, d_init, d_refine, d_ctr = rpd_loss_grads(
            g4, out8, n_refine, logits_buf, init_ltrb, refine_ltrb, ctr_logit, labels, reg_t, ctr_t, sel32, cls, cls_bg, refine_t, loc_strides,
            K, model.focal_loss_alpha, model.focal_loss_gamma, model.iou_loss_type, inv_world, logits_bf16=not f32)
        dctr = torch.zeros((N, L, 8), dtype=HF.ACT_DTYPE, device=dev)
        dctr[:, :, 0] = d_ctr
        # d(LTRB) -> the arg points of the min / max transform, whole rows
        doi, drd = [], []
        for l, (h, w) in enumerate(hw):
            o, ps, shape = offs[l], head.point_strides[l], (N, h, w, ld)
            r32, r16 = HF.points2ltrb_bwd(d_refine.view(-1)[o * 4:], L * 4, refine_arg.view(-1)[o:], L, shape, ps, P, want_f32=f32, want_bf16=not f32)
            d32, _ = HF.points2ltrb_bwd(d_init.view(-1)[o * 4:], L * 4, init_arg.view(-1)[o:], L, shape, ps, P)
            drd.append(r32 if f32 else r16)
            doi.append(d32)
        dl = [dlogits.view(-1)[o * kp:] for o in offs]
        dc = [dctr.view(-1)[o * 8:] for o in offs]
        with GS.wgrad_batch():      # the weight / bias gradient launches of the three prediction convs: one hand-over to the side stream
            HF.conv2d_wgrad_ml(dl, list(cf), arena.grad_view(head.logits.weight), 1, 1, 1, 0, 1, dy_img_stride=L * kp, K=kp, k_real=K)
            arena.mark_ready(head.logits.weight)
            HF.bias_grad(dlogits, arena.grad_view(head.logits.bias), N, L, kp)
            arena.mark_ready(head.logits.bias)
            HF.conv2d_wgrad_ml(drd, list(rf), arena.grad_view(head.offsets_refine.weight), 1, 1, 1, 0, 1)
            arena.mark_ready(head.offsets_refine.weight)
            dbias = arena.grad_view(head.offsets_refine.bias)
            for (h, w), d in zip(hw, drd):
                HF.bias_grad(d, dbias, N, h * w, ld)
            arena.mark_ready(head.offsets_refine.bias)
            HF.conv2d_wgrad_ml(dc, list(ct), arena.grad_view(head.centerness.weight), 3, 3, 1, 1, 1, dy_img_stride=L * 8, K=8, k_real=1)
            arena.mark_ready(head.centerness.weight)
            HF.bias_grad(dctr, arena.grad_view(head.centerness.bias), N, L, 8)
            arena.mark_ready(head.centerness.bias)
        dcf = HF.conv2d_dgrad_ml(dl, head.logits.wt_bf16, hw, 1, 0, 1, dy_img_stride=L * kp, N=N, k_real=K)
        drf = HF.conv2d_dgrad_ml(drd, head.offsets_refine.wt_bf16, hw, 1, 0, 1)
        dct = HF.conv2d_dgrad_ml(dc, head.centerness.wt_bf16, hw, 1, 1, 1, dy_img_stride=L * 8, N=N, k_real=1)
        return (None, None, None, None, None, None, *doi, *dcf, *drf, *dct)


@META_ARCH_REGISTRY.register()
class FCOSRepPoints(FCOSV2):
    """slender_det/modeling/meta_arch/fcos/fcos_rpd_s1_topk.py:137-503; see the module docstring.  Pre-processing, the gt tensors, the
    batched NMS and post-processing are FCOSV2's.  An image without gt is all background in both stages (the reference raises on it)."""
    topk_per_box = 5            # hard-coded at :72

    def __init__(self, cfg):
        if cfg.MODEL.FCOS.NORM_REG_TARGETS:
            raise NotImplementedError(
                "FCOSRepPoints: MODEL.FCOS.NORM_REG_TARGETS is not built: in that mode the reference mixes un-normalised targets with "
                "un-scaled predictions (fcos_rpd_s1_topk.py:338-341 never passes the flag on, :661-666 rectifies the point offsets) and "
                "no config selects it")
        super().__init__(cfg)
        backbone_shape = self.backbone.output_shape()
        self.head = FCOSRepPointsHead(cfg, [backbone_shape[f] for f in self.in_features])
        r = cfg.MODEL.RETINANET                                  # bbox_matcher (:174-178)
        self.iou_thresholds, self.iou_labels = list(r.IOU_THRESHOLDS), list(r.IOU_LABELS)
        self._stride_cache = {}
        self.last_targets = None    # (labels, reg_targets, ctr_targets, stats3) of the last training step, for inspection
        self.last_topk = None       # (N, L) uint8 stage-1 selection
        self.last_refine = None     # (cls, refine_ltrb, matches, match_labels, matched_vals)

    def loc_strides(self, hw):
        """(L,) fp32: the FPN stride of every location (``strides``, :218-220)."""
        key = tuple(hw)
        if key not in self._stride_cache:
            self._stride_cache[key] = torch.cat([torch.full((h * w,), float(s), dtype=torch.float32, device=self.device)
                                                 for (h, w), s in zip(hw, self.fpn_strides)]).contiguous()
        return self._stride_cache[key]

    def losses(self, *args, **kwargs):
        raise NotImplementedError("FCOSRepPoints.losses: the training step computes its losses inside forward() (rpd_loss_sums / rpd_loss_grads "
                                  "on the prediction buffers); the reference's per-level NCHW argument contract is not built")

    @torch.no_grad()
    def get_ground_truth(self, level_hw, gt_instances):
        """Stage 1 (:338-341 + :57-134) for the whole batch: -> labels, reg_targets, slender centerness targets, stats3 = [num_pos, sum of
        the score over the selected rows, the same over all foreground rows], sel (N, L) uint8.  No host read.  Stage 2 (:343-374) needs
        the predicted init boxes and runs inside the loss node."""
        boxes, classes, offs = self._gt_tensors(gt_instances)
        labels, reg_t, ctr_t, _gt_index, sel, stats = HF.fcos_assign_topk(
            boxes, classes, offs, len(gt_instances), level_hw, self.fpn_strides, SIZES_OF_INTEREST, self.center_sampling_radius,
            self.num_classes, self.topk_per_box, slender=True)
        self.last_topk = sel
        return labels, reg_t, ctr_t, stats, sel

    def forward(self, batched_inputs):
        images = self.preprocess_image(batched_inputs)
        if "instances" in batched_inputs[0]:
            gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
        elif "targets" in batched_inputs[0]:
            gt_instances = [x["targets"].to(self.device) for x in batched_inputs]
        else:
            gt_instances = None
        N, Hp, Wp = images.tensor.shape[:3]
        level_hw = [((Hp + s - 1) // s, (Wp + s - 1) // s) for s in self.fpn_strides]
        head = self.head
        if self.training:
            # stage-1 targets first: they depend only on the ground truth, so their all-reduce overlaps the backbone
            targets = self.get_ground_truth(level_hw, gt_instances)
            stats_work = None
            if comm.collectives_active():
                stats_work = dist.all_reduce(targets[3], op=dist.ReduceOp.SUM, async_op=True)
            gt = (*self._gt_tensors(gt_instances), [len(g) for g in gt_instances])
            image_hw = torch.tensor([[float(h), float(w)] for h, w in images.image_sizes], dtype=torch.float32).to(self.device, non_blocking=True)

        features = self.backbone(images.tensor)
        features = [features[f] for f in self.in_features]
        assert [tuple(f.shape[1:3]) for f in features] == level_hw, "feature map sizes differ from the location grid"
        cls_t, box_t = head.run_towers(features)
        oi, cf, rf = head.run_points(cls_t, box_t)
        ctr_in = box_t if head.centerness_on_reg else cls_t
        if self.training:
            if stats_work is not None:
                stats_work.wait()
            l_cls, l_init, l_ref, l_ctr = _FcosRpdLossFn.apply(self, head.logits.weight, targets, gt, image_hw, 1.0 / float(comm.get_world_size()),
                                                               *oi, *cf, *rf, *ctr_in)
            return dict(cls_loss=l_cls, reg_loss_init=l_init, reg_loss=l_ref, centerness_loss=l_ctr)
        results = self.inference(level_hw, oi, cf, rf, ctr_in, images.image_sizes)
        return self.postprocess(results, batched_inputs, images.image_sizes)

    # ------------------------------------------------------------------ inference (:402-477)
    @torch.no_grad()
    def decode_candidates(self, oi, cf, rf, ctr_in):
        """Per-level threshold -> top-k -> linear LTRB decode of the REFINED distances for the whole batch: one kernel, no host sync."""
        logits_buf, ctr_buf, _, _, _, _, refine_ltrb, _, (hw, _, _) = self.head.predict(oi, cf, rf, ctr_in, want_init=False)
        return HF.fcos_decode_ltrb(logits_buf, refine_ltrb, ctr_buf, hw, self.fpn_strides, self.num_classes, self.pre_nms_thresh, self.pre_nms_top_n)

    @torch.no_grad()
    def inference(self, level_hw, oi, cf, rf, ctr_in, image_sizes):
        return self.nms_candidates(self.decode_candidates(oi, cf, rf, ctr_in), image_sizes)
