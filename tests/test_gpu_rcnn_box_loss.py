"""The R-CNN heads' IoU box losses on the GPU (MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE, MODEL.RPN.BBOX_REG_LOSS_TYPE: "giou", "rotated_iou",
"rotated_giou"): the row kernels sod_rows_box_loss_* against the float64 restatement of tests/rcnn_box_loss_restated.py and, bit for
bit, against the RetinaNet kernels that share their loss policies; BBOX_REG_LOSS_WEIGHT; training steps of the small two-stage models
of tests/test_gpu_rcnn.py with each loss on both stages."""
import functools
import math

import pytest
import torch

import rcnn_box_loss_restated as RR
import rotated_giou_loss_restated as GL
import rotated_iou_loss_restated as RL
import test_gpu_rcnn as RC

pytestmark = pytest.mark.gpu

MAX_EXCLUDED = 0.04          # a condition, not a measurement
K3, W5, W4 = 3, RR.W_ROI5, (10.0, 10.0, 5.0, 5.0)
# Four times the values measured on an MI355X against the float64 restatement (the factor covers float32 sinf / cosf differences between
# ROCm versions); the measured values are in the docstring of test_rotated_rows_vs_float64 and are printed on every run.  Conditions on
# top: no row bar above 1e-3, no aggregate bar above 1e-5.
ROW_BAR = {"rotated_iou": 4 * 2.30e-5, "rotated_giou": 4 * 1.64e-6}
AGG_BAR = {"rotated_iou": 4 * 1.96e-6, "rotated_giou": 4 * 5.07e-7}
assert max(ROW_BAR.values()) <= 1e-3 and max(AGG_BAR.values()) <= 1e-5


def _fwd_bar(ref):
    return 1e-4 * max(abs(ref), 1e-3)          # the project's fused-loss bar


# ------------------------------------------------------------------------------------------------ 1. rotated rows
@functools.lru_cache(maxsize=None)
def _rotated_case(kind):
    """The recipe's rows and their float64 reference (computed once per loss, shared, never modified)."""
    pred, labels, src, gt = RR.rotated_rows(192, 192, K3)
    total, g64, fg, boxes = RR.rows_loss(kind, "frcnn", pred, labels, K3, src, gt, W5)
    out = torch.zeros_like(fg)
    out[fg] = GL.excluded(boxes, gt.double()[fg])
    apart = torch.zeros_like(fg)
    apart[fg] = RL.iou(boxes, gt.double()[fg]) == 0
    return pred, labels, src, gt, total, g64, fg, out, apart


@pytest.mark.parametrize("kind", ["rotated_iou", "rotated_giou"])
def test_rotated_rows_vs_float64(cuda, kind):
    """384 Fast R-CNN rows (K = 3, ld = 16: pad column 15; every 7th row background; the other classes' columns hold numbers around 1e3),
    330 of them foreground, 139 of those without overlap with their gt box.  Forward sum within 1e-4 * max(|ref|, 1e-3) of float64
    (measured on an MI355X: rotated_iou 268.2584839 against 268.2584708, rotated_giou 397.2060852 against 397.2060953).  Backward with grad_scale 0.5 on the device and scale_mul 1 / 384 into
    a buffer that held sevens: every foreground row outside the exclusion mask (7 of 330 within 1e-2 px of a kink, 2.1 %; the cap is 4 %)
    against float64 autograd - measured: rotated_iou worst row 2.30e-5 of its norm, all 187 rows together |e| / |ref| = 1.96e-6;
    rotated_giou worst row 1.64e-6, all 323 rows together 5.07e-7; the bars are four times that.  Rows without
    overlap: exactly zero for rotated_iou, non-zero (and compared like the others) for rotated_giou.  Background rows, the other
    classes' columns and the pad column are exactly zero.  R = 1 and R = 257 give the rows of the big call, R = 0 gives sum 0 and
    writes nothing; two calls give the same bits."""
    from slenderobjdet_amd.layers import functional as HF

    pred, labels, src, gt, total, g64, fg, out, apart = _rotated_case(kind)
    R, ld = pred.shape
    p, l, s, g = pred.to(cuda), labels.to(cuda), src.to(cuda), gt.to(cuda)
    got_s = HF.rows_box_loss_fwd(kind, "frcnn", p, l, K3, s, g, W5, RR.SCALE_CLAMP)
    again = HF.rows_box_loss_fwd(kind, "frcnn", p, l, K3, s, g, W5, RR.SCALE_CLAMP)
    print(f"\n{kind}: forward sum hip {float(got_s):.7f} float64 {total:.7f} (|e| {abs(float(got_s) - total):.3g}, bar {_fwd_bar(total):.3g})")
    assert got_s.shape == (1,) and torch.equal(got_s, again)
    assert abs(float(got_s) - total) <= _fwd_bar(total)
    half = torch.full((1,), 0.5, device=cuda)
    d = torch.full((R, ld), 7.0, device=cuda)
    ret = HF.rows_box_loss_bwd(kind, "frcnn", p, l, K3, s, g, W5, RR.SCALE_CLAMP, half, 1.0 / R, out=d)
    assert ret is d
    d2 = HF.rows_box_loss_bwd(kind, "frcnn", p, l, K3, s, g, W5, RR.SCALE_CLAMP, half, 1.0 / R)
    assert torch.equal(d, d2)
    got = d.cpu().double()
    ref = g64 * (0.5 / R)
    # exact zeros: background rows, the other classes' columns, the pad column
    own = torch.zeros(R, ld, dtype=torch.bool)
    cols = labels.long()[fg, None] * 5 + torch.arange(5)[None]
    own[fg] = own[fg].scatter(1, cols, torch.ones_like(cols, dtype=torch.bool))
    assert (got[~own] == 0).all() and (ref[~own] == 0).all() and (got[:, 15] == 0).all() and (got[~fg] == 0).all()
    share = float(out[fg].double().mean())
    assert share <= MAX_EXCLUDED
    keep = fg & ~out
    if kind == "rotated_iou":
        assert int((fg & apart).sum()) > 100 and (got[apart] == 0).all() and (ref[apart] == 0).all()
        keep = keep & ~apart
    else:
        assert int((keep & apart).sum()) > 100 and bool((got[keep & apart].norm(dim=1) > 0).all())
    e = got - ref
    row = e.norm(dim=1)[keep] / ref.norm(dim=1)[keep]
    agg = float(e[keep].norm() / ref[keep].norm())
    worst = int(torch.nonzero(keep)[row.argmax(), 0])
    print(f"{kind}: {int(fg.sum())} foreground rows, {int(out[fg].sum())} left out ({100 * share:.2f} %), {int((fg & apart).sum())} without overlap, "
          f"{int(keep.sum())} compared: worst row {float(row.max()):.3g} of its norm (row {worst}), all rows |e| / |ref| = {agg:.3g} "
          f"(bars {ROW_BAR[kind]:.3g}, {AGG_BAR[kind]:.3g})")
    assert int(keep.sum()) >= 150
    assert float(row.max()) <= ROW_BAR[kind] and agg <= AGG_BAR[kind]
    for n in (1, 257):
        dn = HF.rows_box_loss_bwd(kind, "frcnn", p[:n].contiguous(), l[:n].contiguous(), K3, s[:n].contiguous(), g[:n].contiguous(), W5,
                                  RR.SCALE_CLAMP, half, 1.0 / R)
        assert torch.equal(dn, d[:n])
        sn = HF.rows_box_loss_fwd(kind, "frcnn", p[:n].contiguous(), l[:n].contiguous(), K3, s[:n].contiguous(), g[:n].contiguous(), W5, RR.SCALE_CLAMP)
        want, _, _, _ = RR.rows_loss(kind, "frcnn", pred[:n], labels[:n], K3, src[:n], gt[:n], W5)
        assert abs(float(sn) - want) <= _fwd_bar(want), (n, float(sn), want)
    s0 = HF.rows_box_loss_fwd(kind, "frcnn", p[:0].contiguous(), l[:0].contiguous(), K3, s[:0].contiguous(), g[:0].contiguous(), W5, RR.SCALE_CLAMP)
    d0 = HF.rows_box_loss_bwd(kind, "frcnn", p[:0].contiguous(), l[:0].contiguous(), K3, s[:0].contiguous(), g[:0].contiguous(), W5, RR.SCALE_CLAMP,
                              half, 1.0)
    assert float(s0) == 0.0 and d0.shape == (0, ld)


# ------------------------------------------------------------------------------------------------ 2. RPN rows == the RetinaNet kernels
@pytest.mark.parametrize("kind, stem", [("rotated_iou", "riou"), ("rotated_giou", "rgiou")])
def test_rpn_rows_equal_the_retina_kernels_bit_for_bit(cuda, kind, stem):
    """The same numbers as RPN rows (int8 labels, ld = 5) and as a RetinaNet buffer (N = 1, A = 1, pitch = 5; label 1 -> class 0,
    everything else -> num_classes): both kernels call one definition of the loss policy, so with both scales 1 the delta gradients are
    torch.equal in fp32 mode; the sums agree to 1e-6 relative (the reduction orders differ)."""
    from slenderobjdet_amd.layers import functional as HF

    pred, labels, src, gt, _, _, fg, _, _ = _rotated_case(kind)
    R = pred.shape[0]
    cols = (labels.long() % K3)[:, None] * 5 + torch.arange(5)[None]
    rows5 = torch.gather(pred, 1, cols).contiguous()
    lab8 = torch.where(fg, 1, torch.where(torch.arange(R) % 2 == 0, 0, -1)).to(torch.int8)
    lab32 = torch.where(fg, 0, 1).to(torch.int32)
    p, s, g = rows5.to(cuda), src.to(cuda), gt.to(cuda)
    one = torch.ones(1, device=cuda)
    s_rows = HF.rows_box_loss_fwd(kind, "rpn", p, lab8.to(cuda), 1, s, g, W5, RR.SCALE_CLAMP)
    d_rows = torch.full((R, 5), 7.0, device=cuda)
    HF.rows_box_loss_bwd(kind, "rpn", p, lab8.to(cuda), 1, s, g, W5, RR.SCALE_CLAMP, one, 1.0, out=d_rows)
    prev = HF.set_precision("fp32")
    try:
        fwd, bwd = getattr(HF, f"retina_{stem}_loss_fwd"), getattr(HF, f"retina_{stem}_loss_bwd")
        sums = fwd(p.view(1, R, 5), 5, lab32.to(cuda).view(1, R), s, g.view(1, R, 5), 1, R, 1, 1, W5, RR.SCALE_CLAMP, one.clone(), 0.9)
        d_ret = torch.full((1, R, 5), 7.0, dtype=HF.ACT_DTYPE, device=cuda)
        assert d_ret.dtype == torch.float32
        bwd(p.view(1, R, 5), 5, lab32.to(cuda).view(1, R), s, g.view(1, R, 5), 1, R, 1, 1, W5, RR.SCALE_CLAMP, one, one, d_ret)
    finally:
        HF.set_precision(prev)
    rel = abs(float(s_rows) - float(sums[0])) / float(sums[0])
    print(f"\n{kind}: rows sum {float(s_rows):.7f}, retina sum {float(sums[0]):.7f} (rel {rel:.3g}), {int(sums[1])} positives")
    assert int(sums[1]) == int(fg.sum()) and rel <= 1e-6
    assert torch.equal(d_rows, d_ret.view(R, 5))
    assert (d_rows[~fg.to(cuda)] == 0).all() and d_rows[fg.to(cuda)].abs().sum() > 0
    # and the Fast R-CNN rows of the same numbers are the same bits again, in their class's columns
    d_frcnn = HF.rows_box_loss_bwd(kind, "frcnn", pred.to(cuda), labels.to(cuda), K3, s, g, W5, RR.SCALE_CLAMP, one, 1.0)
    assert torch.equal(torch.gather(d_frcnn, 1, cols.to(cuda))[fg.to(cuda)], d_rows[fg.to(cuda)])


# ------------------------------------------------------------------------------------------------ 3. GIoU rows
K5, LD5 = 5, 24


@functools.lru_cache(maxsize=None)
def _giou_case():
    """256 axis-aligned rows: gt boxes (centre U(20, 200), sides U(8, 80)); the wanted box = the gt with its corners moved by N(0, 2),
    for every 4th row also 100 px away (no overlap: the enclosing-box term alone acts); the proposal = the wanted box jittered (centre
    +- 10 % of its sides, sides x exp(+- 0.2)); deltas = get_deltas(proposal, wanted) in float64, rounded to float32.  K = 5, ld = 24
    (pad columns 20 .. 23); the class cycles 0 .. 4, every 6th row is background, row 3 is ignored (-1).  The first foreground row has
    its dw pushed to 25 (25 / 5 = 5 > log(1000 / 16))."""
    g = torch.Generator().manual_seed(23)
    R = 256
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    c, wh = 20 + 180 * u(R, 2), 8 + 72 * u(R, 2)
    gt = torch.cat([c - wh / 2, c + wh / 2], 1).float().double()
    wanted = gt + 2.0 * torch.randn(R, 4, generator=g, dtype=torch.float64)
    wanted[3::4] += 100.0
    wc, wwh = (wanted[:, :2] + wanted[:, 2:]) / 2, wanted[:, 2:] - wanted[:, :2]
    assert float(wwh.min()) > 1.0
    pc, pwh = wc + (u(R, 2) - 0.5) * 0.2 * wwh, wwh * torch.exp((u(R, 2) - 0.5) * 0.4)
    src = torch.cat([pc - pwh / 2, pc + pwh / 2], 1).float().double()
    deltas = RR.get_deltas_xyxy(src, wanted, W4).float()
    labels = (torch.arange(R) % K5).to(torch.int32)
    labels[5::6] = K5
    labels[3] = -1
    deltas[0, 2] = 25.0
    pred = (torch.randn(R, LD5, generator=g, dtype=torch.float64) * 1e3).float()
    fg = (labels >= 0) & (labels < K5)
    cols = labels.long().clamp(0, K5 - 1)[:, None] * 4 + torch.arange(4)[None]
    pred[fg] = pred[fg].scatter(1, cols[fg], deltas[fg])
    return pred, labels, src.float(), gt.float(), deltas, fg, cols


@pytest.mark.parametrize("rows", ["frcnn", "rpn"])
def test_giou_rows_vs_float64(cuda, rows):
    """Fast R-CNN rows (K = 5, ld = 24) and the same deltas as RPN rows (ld = 4).  Forward within 1e-4 * max(|ref|, 1e-3) of float64;
    the foreground rows together within 2e-6 of their norm of float64 autograd (the project's fp32 bar of
    test_retinanet_giou_backward_rows_vs_float64); the clamped dw has gradient exactly 0 while its row is not zero; everything that
    is not a foreground row's own column is exactly zero in a buffer that held sevens.  The RPN rows equal sod_retina_giou_loss_bwd_f32
    (N = 1, A = 1, pitch 4) bit for bit."""
    from slenderobjdet_amd.layers import functional as HF

    pred, labels, src, gt, deltas, fg, cols = _giou_case()
    R = pred.shape[0]
    if rows == "rpn":
        pred, labels, K = deltas.contiguous(), torch.where(fg, 1, torch.where(torch.arange(R) % 2 == 0, 0, -1)).to(torch.int8), 1
        cols = torch.arange(4)[None].expand(R, -1)
    else:
        K = K5
    ld = pred.shape[1]
    total, g64, fg2, boxes = RR.rows_loss("giou", rows, pred, labels, K, src, gt, W4)
    assert torch.equal(fg2, fg) and fg[0] and int(fg.sum()) > 200
    w0 = float(src[0, 2] - src[0, 0])
    assert abs(float(boxes[0, 2] - boxes[0, 0]) / w0 - 62.5) < 1e-3          # the clamp is active: exp(log(1000 / 16))
    p, l, s, g = pred.to(cuda), labels.to(cuda), src.to(cuda), gt.to(cuda)
    got_s = HF.rows_box_loss_fwd("giou", rows, p, l, K, s, g, W4, RR.SCALE_CLAMP)
    print(f"\ngiou {rows}: forward sum hip {float(got_s):.7f} float64 {total:.7f}")
    assert abs(float(got_s) - total) <= _fwd_bar(total)
    one = torch.ones(1, device=cuda)
    d = torch.full((R, ld), 7.0, device=cuda)
    HF.rows_box_loss_bwd("giou", rows, p, l, K, s, g, W4, RR.SCALE_CLAMP, one, 1.0 / R, out=d)
    got, ref = d.cpu().double(), g64 / R
    own = torch.zeros(R, ld, dtype=torch.bool)
    own[fg] = own[fg].scatter(1, cols[fg], torch.ones(int(fg.sum()), 4, dtype=torch.bool))
    assert (got[~own] == 0).all() and (ref[~own] == 0).all() and (got[:, K * 4:] == 0).all()
    e = (got - ref)[fg]
    agg = float(e.norm() / ref[fg].norm())
    print(f"giou {rows}: delta-gradient rows of {int(fg.sum())} foreground rows off by {agg:.3g} of their norm together (bar 2e-6)")
    assert agg <= 2e-6
    c0 = int(cols[0, 0])
    assert got[0, c0 + 2] == 0 and ref[0, c0 + 2] == 0 and got[0, c0:c0 + 4].abs().sum() > 0
    if rows == "rpn":
        d1 = HF.rows_box_loss_bwd("giou", rows, p, l, K, s, g, W4, RR.SCALE_CLAMP, one, 1.0)
        lab32 = torch.where(fg, 0, 1).to(torch.int32).to(cuda)
        prev = HF.set_precision("fp32")
        try:
            d_ret = torch.full((1, R, 4), 7.0, dtype=HF.ACT_DTYPE, device=cuda)
            HF.retina_giou_loss_bwd(p.view(1, R, 4), 4, lab32.view(1, R), s, g.view(1, R, 4), 1, R, 1, 1, W4, RR.SCALE_CLAMP, one, one, d_ret)
        finally:
            HF.set_precision(prev)
        assert d_ret.dtype == torch.float32 and torch.equal(d1, d_ret.view(R, 4))


# ------------------------------------------------------------------------------------------------ 4. loss weight
def test_box_reg_loss_weight_doubles_loss_and_gradient(cuda):
    """Two FastRCNNOutputLayers that differ only in BBOX_REG_LOSS_WEIGHT (1.0 and 2.0) on the same fixed predictions and proposals:
    loss_box_reg and the delta gradient are exactly doubled (a power of two), loss_cls is untouched."""
    from slenderobjdet_amd.modeling.box_regression import Box2BoxTransformRotated
    from slenderobjdet_amd.modeling.roi_heads.roi_heads import FastRCNNOutputLayers
    from slenderobjdet_amd.structures import Instances, RotatedBoxes

    pred, labels, src, gt, _, _, fg, _, _ = _rotated_case("rotated_giou")
    R = pred.shape[0]
    out = {}
    for weight in (1.0, 2.0):
        cfg = RC._cfg(True)
        cfg.MODEL.ROI_HEADS.NUM_CLASSES = K3
        cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = "rotated_giou"
        cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT = weight
        torch.manual_seed(0)
        layer = FastRCNNOutputLayers(cfg, 64, Box2BoxTransformRotated(weights=W5)).to(cuda)
        assert layer.box_out == 16 and layer.cls_pad == 8 and layer.box_reg_loss_weight == weight
        scores = torch.randn(R, 1, 1, 8, generator=torch.Generator().manual_seed(5)).to(cuda).requires_grad_(True)
        deltas = pred.to(cuda).view(R, 1, 1, 16).clone().requires_grad_(True)
        props = []
        for lo, hi in ((0, 200), (200, R)):
            inst = Instances((128, 128))
            inst.proposal_boxes = RotatedBoxes(src[lo:hi].to(cuda))
            inst.gt_boxes = RotatedBoxes(gt[lo:hi].to(cuda))
            inst.gt_classes = labels[lo:hi].long().to(cuda)
            props.append(inst)
        losses = layer.losses((scores, deltas), props)
        assert sorted(losses) == ["loss_box_reg", "loss_cls"]
        (losses["loss_cls"] + losses["loss_box_reg"]).backward()
        out[weight] = (losses["loss_cls"].detach(), losses["loss_box_reg"].detach(), scores.grad.clone(), deltas.grad.clone())
    (c1, b1, gs1, gd1), (c2, b2, gs2, gd2) = out[1.0], out[2.0]
    total, _, _, _ = RR.rows_loss("rotated_giou", "frcnn", pred, labels, K3, src, gt, W5)
    print(f"\nloss_box_reg weight 1: {float(b1):.7f} (float64 {total / R:.7f}), weight 2: {float(b2):.7f}")
    assert abs(float(b1) - total / R) <= _fwd_bar(total / R)
    assert torch.equal(c1, c2) and torch.equal(gs1, gs2)
    assert torch.equal(b2, b1 * 2.0) and torch.equal(gd2, gd1 * 2.0) and gd1.abs().sum() > 0


# ------------------------------------------------------------------------------------------------ 5. model steps
def _step_with(rotated, kind, mode, cuda):
    from bench import damp_residual_branches
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.solver import build_optimizer

    prev = HF.set_precision(mode)
    try:
        cfg = RC._cfg(rotated)
        cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = kind
        cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE = kind
        torch.manual_seed(0)
        model = build_model(cfg)
        model.train()
        damp_residual_branches(model)          # see the docstring of the test
        opt = build_optimizer(cfg, model)
        data = RC._data(2, 96, 128, 21, rotated)
        cap = {}
        hooks = [model.roi_heads.box_predictor.register_forward_hook(lambda m, i, o: cap.__setitem__("roi", o[1].detach().clone())),
                 model.proposal_generator.head.register_forward_hook(lambda m, i, o: cap.__setitem__("rpn", [x.detach().clone() for x in o[1]]))]
        got = model(data)
        for h in hooks:
            h.remove()
        total = sum(got.values())
        opt.zero_grad()
        model.arena.begin_backward(); total.backward(); model.arena.finish_backward()
        torch.cuda.synchronize()
    finally:
        HF.set_precision(prev)
    return model, got, cap


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("rotated, kind", [(False, "giou"), (True, "rotated_iou"), (True, "rotated_giou")])
def test_training_step_with_the_iou_losses_on_both_stages(cuda, rotated, kind, mode):
    """One step of the R18 two-stage model of tests/test_gpu_rcnn.py (2 images of 96 x 128, data seed 21) with the loss on both stages,
    in the bf16 product path and in fp32 mode.  The box predictor's deltas (a forward hook) and ``roi_heads.last_proposals``, the RPN
    head's deltas gathered at ``RPN.last_sampled`` - the numbers the kernels read - go through the float64 restatement: loss_box_reg =
    sum / number of sampled rows and loss_rpn_loc = sum / (BATCH_SIZE_PER_IMAGE * N), both within 1e-4 * max(|ref|, 1e-3).  The loss
    keys are unchanged, every trainable parameter has a finite gradient, the real rows of bbox_pred's and of the RPN's anchor_deltas'
    weight gradient are non-zero and the pad rows exactly zero.
    The residual branches are damped as in bench.py and test_rotated_rcnn_r101_step: a random-init body without normalisation statistics
    drives the untrained heads with features around 1e3, and their deltas (up to +- 20) decode to slivers - measured here without the
    damping: an RPN row decoded to 8000 x 1.5e-5 px, for which the fp32 clipping of rotated_iou.h (detectron2's algorithm, the number NMS
    and the matcher see, and what sod_rotated_iou_loss returns for the same pair) gives an IoU of 1.0e5 where float64 geometry gives 0.
    The loss inherits that number by definition; a comparison with float64 geometry is only meaningful on boxes the clipping resolves."""
    model, got, cap = _step_with(rotated, kind, mode, cuda)
    assert set(got) == {"loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg"}
    assert all(math.isfinite(float(v)) for v in got.values()), got
    D = 5 if rotated else 4
    rpn, roi = model.proposal_generator, model.roi_heads
    assert rpn.box_reg_loss_type == roi.box_predictor.box_reg_loss_type == kind
    # Fast R-CNN rows
    props = roi.last_proposals
    R = sum(len(p) for p in props)
    deltas = cap["roi"].view(R, -1).cpu()
    cls = torch.cat([p.gt_classes for p in props]).to(torch.int32).cpu()
    boxes = torch.cat([p.proposal_boxes.tensor for p in props]).cpu()
    gtb = torch.cat([p.gt_boxes.tensor for p in props]).cpu()
    t = roi.box_predictor.box2box_transform
    total, _, fg, _ = RR.rows_loss(kind, "frcnn", deltas, cls, 80, boxes, gtb, t.weights)
    ref_box = total / max(R, 1)
    # RPN rows
    idx, labels_s, (src_s, gt_s) = rpn.last_sampled
    A, N, S = rpn.head.num_anchors, idx.shape[0], rpn.batch_size_per_image
    flat = torch.cat([x[..., :A * D].reshape(N, -1, D) for x in cap["rpn"]], 1)
    rows = torch.gather(flat, 1, idx.clamp(min=0).long()[:, :, None].expand(-1, -1, D)).reshape(-1, D).cpu()
    total_r, _, fg_r, _ = RR.rows_loss(kind, "rpn", rows, labels_s.view(-1).cpu(), 1, src_s.reshape(-1, D).cpu(), gt_s.reshape(-1, D).cpu(),
                                       rpn.box2box_transform.weights)
    ref_loc = total_r / (S * N) * rpn.loss_weight["loss_rpn_loc"]
    a_box, a_loc = float(got["loss_box_reg"].detach()), float(got["loss_rpn_loc"].detach())
    print(f"\n{kind} {mode}: loss_box_reg hip {a_box:.7f} restated {ref_box:.7f} ({int(fg.sum())} of {R} rows foreground); "
          f"loss_rpn_loc hip {a_loc:.7f} restated {ref_loc:.7f} ({int(fg_r.sum())} of {S * N} sampled anchors positive)")
    assert int(fg.sum()) >= 2 and int(fg_r.sum()) >= 2
    assert abs(a_box - ref_box) <= _fwd_bar(ref_box)
    assert abs(a_loc - ref_loc) <= _fwd_bar(ref_loc)
    n = 0
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            n += 1
    assert n > 30
    gw = roi.box_predictor.bbox_pred.weight.grad
    assert gw.shape[0] == roi.box_predictor.box_out and gw[:80 * D].abs().sum() > 0 and (gw[80 * D:] == 0).all()
    ga = rpn.head.anchor_deltas.conv.weight.grad
    assert ga.shape[0] == rpn.head.delta_pad > A * D and ga[:A * D].abs().sum() > 0 and (ga[A * D:] == 0).all()
