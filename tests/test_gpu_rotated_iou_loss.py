"""The rotated IoU loss on the GPU: the pair operator (forward bit-equal to box_iou_rotated, backward against float64 autograd of the
restatement in tests/rotated_iou_loss_restated.py), the labeller's matched-box variant, the fused RetinaNet form and a training step
of RotatedRetinaNet with MODEL.RETINANET.BBOX_REG_LOSS_TYPE "rotated_iou"."""
import math

import pytest
import torch

import rotated_iou_loss_restated as RL
import rotated_retinanet_restated as RS

pytestmark = pytest.mark.gpu

K8 = 8
W5 = (1.0, 1.0, 1.0, 1.0, 1.0)
THR, LAB = [0.4, 0.5], [0, -1, 1]
MARGIN, MAX_EXCLUDED = 1e-2, 0.03
# Four times the values measured on an MI355X (the factor covers float32 sinf / cosf differences between ROCm versions); the measured
# values are in the docstrings of the tests that use them and are printed on every run.
PAIR_ROW_BAR, PAIR_AGG_BAR = 4 * 1.03e-4, 4 * 1.07e-6
FUSED_ROW_BAR, FUSED_AGG_BAR = 4 * 1.16e-5, 4 * 2.38e-7


def _pairs(count, seed):
    """generate(count, seed) plus the special cases, rounded to float32 (what the kernel sees) -> float64 pred, gt and the masks."""
    p, g = RL.generate(count, seed)
    sp, sg, forward_only, names = RL.special_cases()
    pred, gt = torch.cat([p, sp]).float().double(), torch.cat([g, sg]).float().double()
    fo = torch.cat([torch.zeros(count, dtype=torch.bool), forward_only])
    return pred, gt, fo, names


# ------------------------------------------------------------------------------------------------ 1. pair forward
def test_pair_forward_is_box_iou_rotated(cuda):
    """elem_out = 1 - IoU with the IoU of HF.box_iou_rotated on the same boxes, to the bit: ``elem == 1 - diag`` in float32 for every
    row, and ``1 - elem == diag`` wherever the subtraction is exact (IoU >= 0.5; below that 1 - IoU drops low bits of the IoU, so the
    round trip cannot return them).  Against the float64 restatement: 2e-4, the bar test_box_iou_rotated_known_values_and_oracle
    (test_gpu_detection_ops.py) holds box_iou_rotated to against its oracle (measured on an MI355X: 1.1e-6).  sum_out against the
    sum of the float32 elements: 1e-6 relative (measured 2.8e-8).  P = 1 and P = 257 (one lane over a workgroup) work; P = 0 gives 0."""
    from slenderobjdet_amd.layers import functional as HF

    pred, gt, _, names = _pairs(512, 3)
    a, b = pred.float().to(cuda), gt.float().to(cuda)
    elem, s = HF.rotated_iou_loss_fwd(a, b)
    diag = HF.box_iou_rotated(a, b).diagonal().contiguous()
    assert torch.equal(elem, 1.0 - diag)
    hi = diag >= 0.5
    assert int(hi.sum()) > 100 and torch.equal((1.0 - elem)[hi], diag[hi])
    ref = RL.iou(pred, gt)
    err = float(((1.0 - elem.cpu().double()) - ref).abs().max())
    want = float(elem.double().sum())
    rel = abs(float(s) - want) / want
    print(f"\npair forward: {elem.numel()} pairs, max |IoU - float64| {err:.3g}, sum {float(s):.7f} against {want:.7f} (rel {rel:.3g})")
    assert err <= 2e-4
    assert rel <= 1e-6
    sp = dict(zip(names, (1.0 - elem[512:]).tolist()))
    assert sp["disjoint"] == 0.0 and abs(sp["identical"] - 1.0) < 1e-5 and abs(sp["swapped_90"] - 1.0) < 1e-4
    for P in (1, 257):
        e2, s2 = HF.rotated_iou_loss_fwd(a[:P].contiguous(), b[:P].contiguous())
        assert torch.equal(e2, elem[:P]) and abs(float(s2) - float(elem[:P].double().sum())) <= 1e-6 * max(float(elem[:P].double().sum()), 1e-3)
    e0, s0 = HF.rotated_iou_loss_fwd(a[:0].contiguous(), b[:0].contiguous())
    assert e0.numel() == 0 and float(s0) == 0.0


# ------------------------------------------------------------------------------------------------ 2. pair backward
def test_pair_backward_vs_float64_autograd(cuda):
    """d (1 - IoU) / d pred of 4 096 generated pairs and the special cases against float64 autograd of the restatement.  Rows whose
    forward IoU is 0 are exactly zero (and disjoint in float64); rows closer than 1e-2 px to a change of the intersection's structure
    (margin) and the forward-only special cases are left out, at most 3 % (measured 57 of 4 106, 1.39 %; 69 rows without overlap).
    Measured on an MI355X over the other 3 980 rows: worst row off by 1.03e-4 of its norm (a pair with IoU below 1e-4, where the
    gradient itself is tiny), all rows together |e| / |ref| = 1.07e-6; the bars are four times that.  grad_scale is linear: 0.25
    gives exactly a quarter; the autograd function (sum / mean / none) returns the same numbers."""
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.layers import rotated_iou_loss

    pred, gt, fo, names = _pairs(4096, 5)
    a, b = pred.float().to(cuda), gt.float().to(cuda)
    elem, _ = HF.rotated_iou_loss_fwd(a, b)
    d = HF.rotated_iou_loss_bwd(a, b)
    ref_l, ref_g = RL.loss_and_grad(pred, gt)
    zero = (elem == 1.0).cpu()
    got = d.cpu().double()
    assert int(zero.sum()) > 20 and (got[zero] == 0).all() and (ref_l[zero] >= 1.0 - 1e-6).all()
    assert zero[4096 + names.index("disjoint")]
    out = ((RL.margin(pred, gt) < MARGIN) | fo) & ~zero
    share = float(out.double().mean())
    keep = ~out & ~zero
    e = got - ref_g
    row = (e.norm(dim=1) / ref_g.norm(dim=1))[keep]
    agg = float(e[keep].norm() / ref_g[keep].norm())
    worst = int(torch.nonzero(keep)[row.argmax(), 0])
    print(f"\npair backward: {int(zero.sum())} rows without overlap, {int(out.sum())} left out ({100 * share:.2f} %), {int(keep.sum())} compared: "
          f"worst row {float(row.max()):.3g} of its norm (pair {worst}, IoU {1 - float(ref_l[worst]):.4f}), all rows |e| / |ref| = {agg:.3g}")
    assert share <= MAX_EXCLUDED
    assert keep[4096:].sum() == len(names) - int(fo.sum()) - 1          # every special case with a gradient is compared
    assert float(row.max()) <= PAIR_ROW_BAR and agg <= PAIR_AGG_BAR
    d1 = HF.rotated_iou_loss_bwd(a, b, grad_scale=torch.ones(1, device=cuda))
    dq = HF.rotated_iou_loss_bwd(a, b, grad_scale=torch.full((1,), 0.25, device=cuda))
    assert torch.equal(d1, d) and torch.equal(dq, d * 0.25)
    # the autograd function
    for reduction in ("sum", "mean", "none"):
        ar = a.clone().requires_grad_(True)
        l = rotated_iou_loss(ar, b, reduction=reduction)
        if reduction == "none":
            assert torch.equal(l, elem)
            l.sum().backward()
            assert torch.equal(ar.grad, d)
        else:
            want = float(elem.double().sum()) / (a.shape[0] if reduction == "mean" else 1)
            assert abs(float(l.detach()) - want) <= 1e-6 * want
            (l * 2.0).backward()
            scale = 2.0 / (a.shape[0] if reduction == "mean" else 1)
            assert float((ar.grad - d * scale).abs().max()) <= 1e-6 * scale * float(d.abs().max())


# ------------------------------------------------------------------------------------------------ 3. labeller variant
def _padded(boxes, classes, dev):
    N, Gmax = len(boxes), max(len(b) for b in boxes)
    pb = torch.zeros(N, Gmax, 5)
    pc = torch.zeros(N, Gmax, dtype=torch.int32)
    for i, (b, c) in enumerate(zip(boxes, classes)):
        pb[i, : len(b)], pc[i, : len(b)] = b, c.to(torch.int32)
    cnt = torch.tensor([len(b) for b in boxes], dtype=torch.int32)
    return pb.to(dev), pc.to(dev), cnt.to(dev)


@pytest.mark.parametrize("counts", [(0, 7), (1, 7)])
def test_labeller_returns_the_matched_boxes(cuda, counts):
    """retina_label_rotated(want_boxes=True): labels torch.equal to the delta variant's; matched_boxes = gt_boxes[match] for EVERY anchor
    (positive or not), the match being sod_anchor_match_rotated's; zeros for an image without gts.  282 anchors: one full 256-anchor
    chunk and a partial one."""
    from slenderobjdet_amd.layers import functional as HF

    g = torch.Generator().manual_seed(17 + counts[0])
    anc = RS.anchors([(5, 7), (3, 4)], [8, 16], [[32], [64]], [[1.0, 4.0]], [[-60, 0, 60]])
    assert anc.shape == (282, 5)
    boxes, classes = [], []
    for n in counts:
        boxes.append(torch.stack([torch.rand(n, generator=g) * 56, torch.rand(n, generator=g) * 40, 12 + torch.rand(n, generator=g) * 52,
                                  4 + torch.rand(n, generator=g) * 20, torch.rand(n, generator=g) * 360 - 180], 1))
        classes.append(torch.randint(0, K8, (n,), generator=g))
    A = anc.to(cuda)
    pb, pc, cnt = _padded(boxes, classes, cuda)
    lab_d, deltas = HF.retina_label_rotated(A, pb, pc, cnt, THR, LAB, True, K8, W5)
    lab_b, mb = HF.retina_label_rotated(A, pb, pc, cnt, THR, LAB, True, K8, W5, want_boxes=True)
    assert torch.equal(lab_b, lab_d) and mb.shape == (2, 282, 5)
    pos = (lab_b >= 0) & (lab_b != K8)
    assert int(pos[1].sum()) > 0
    for i, b in enumerate(boxes):
        if len(b) == 0:
            assert (mb[i] == 0).all() and (lab_b[i] == K8).all()
            continue
        _, idx, _ = HF.anchor_match(b.to(cuda), A, THR, LAB, True)
        assert torch.equal(mb[i], b.to(cuda)[idx.long()])
    # the deltas of the other entry point are the deltas towards these very boxes
    ref_d = HF.box2box_get_deltas(A, mb[1].contiguous(), W5)
    assert float((deltas[1] - ref_d).abs().max()) <= 1e-5
    lab_n, mb_n = HF.retina_label_rotated(A, pb, pc, cnt, THR, LAB, False, K8, W5, want_boxes=True)       # one launch, no promotion
    assert torch.equal(mb_n, mb) and torch.equal(lab_n, HF.retina_label_rotated(A, pb, pc, cnt, THR, LAB, False, K8, W5)[0])


# ------------------------------------------------------------------------------------------------ the R18 model
def _cfg(box_loss):
    """R18-FPN RotatedRetinaNet with A = 6, K = 8: 48 class channels, 30 deltas in a 32-wide buffer."""
    from bench import make_cfg

    cfg = make_cfg(18)
    cfg.MODEL.META_ARCHITECTURE = "RotatedRetinaNet"
    ag = cfg.MODEL.ANCHOR_GENERATOR
    ag.NAME = "RotatedAnchorGenerator"
    ag.SIZES = [[32], [64], [128], [256], [512]]
    ag.ASPECT_RATIOS = [[1.0, 4.0]]
    ag.ANGLES = [[-60, 0, 60]]
    cfg.MODEL.RETINANET.BBOX_REG_WEIGHTS = W5
    cfg.MODEL.RETINANET.NUM_CLASSES = K8
    cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = box_loss
    return cfg


def _data(n, h, w, seed, num_classes):
    from slenderobjdet_amd.data import synthetic_batch

    return synthetic_batch(n, h, w, seed, num_classes=num_classes, device="cuda", rotated=True)


def _buffers(model, data):
    with torch.no_grad():
        imgs = model.preprocess_image(data)
        feats = model.backbone(imgs.tensor)
        feats = [feats[f] for f in model.in_features]
        hw = [tuple(f.shape[1:3]) for f in feats]
        ct, bt = model.head.run_towers(feats)
        cls_buf, box_buf, _, offs = model.head.predict(ct, bt)
    return imgs, hw, cls_buf, box_buf, offs


def _restated_box_loss(pdel, anchors, matched, pos, weights):
    """sum over the positives of 1 - IoU(decode(deltas, anchor), matched gt) in float64 and its gradient w.r.t. the deltas (N, R, 5)."""
    N, R = pos.shape
    pd = pdel.double().clone().requires_grad_(True)
    anc = anchors.double()[None].expand(N, -1, -1)
    boxes = RL.decode(pd[pos], anc[pos], weights)
    total = (1.0 - RL.iou(boxes, matched.double()[pos])).sum()
    (g,) = torch.autograd.grad(total, pd)
    return float(total.detach()), g, boxes.detach()


# ------------------------------------------------------------------------------------------------ 4. fused form
def test_fused_loss_vs_restatement(cuda):
    """sod_retina_riou_loss_* on the R18 model's own prediction buffer, labels and matched boxes (2 images of 128 x 160, A = 6, K = 8,
    pitch 32).  loss_box_reg of the model within 1e-4 * max(|ref|, 1e-3) of the restatement chained through float64 apply_deltas, the
    EMA normaliser within 1e-3.  Then, with the dw of one positive pushed above the clamp: the sum again, and the gradient rows of the
    positives against float64 autograd - bf16 storage 4e-3 of their norm together (the bf16 storage bar of
    test_loss_kernels_vs_restatement; measured 1.79e-3), fp32 storage four times the values measured on an MI355X (worst row 1.16e-5
    of its norm, all rows 2.38e-7); rows closer than 1e-2 px to a kink are left out, at most 3 % (measured 0 of 63).  6 of the 63
    positives (low-quality matches) do not overlap their gt once decoded: loss 1 each, gradient rows exactly zero, like every
    non-positive row and the pad columns - in a buffer that held sevens.  The clamped dw has gradient exactly 0 while its row is not
    zero.  Measured: loss_box_reg 0.5598356 against 0.5598356; clamped sum 53.9737244 against 53.9737240."""
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.modeling import build_model

    cfg = _cfg("rotated_iou")
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    A, K, pitch = model.head.num_anchors, model.num_classes, model.head.box_pitch
    assert (A, K, pitch) == (6, K8, 32)
    data = _data(2, 128, 160, 21, K)
    _, hw, _, box_buf, _ = _buffers(model, data)
    anchors = model.anchors_for(hw)
    lab, matched = model.label_anchors(anchors, [d["instances"] for d in data])
    N, P = box_buf.shape[:2]
    R = P * A
    assert matched.shape == (N, R, 5)
    pos = ((lab >= 0) & (lab != K)).cpu()
    npos = int(pos.sum())
    assert npos >= 10 and int((~pos).sum()) > 0
    pdel = box_buf.cpu()[..., : A * 5].reshape(N, R, 5)
    total, _, _ = _restated_box_loss(pdel, anchors.cpu(), matched.cpu(), pos, W5)
    norm = 0.9 * 100.0 + 0.1 * max(npos, 1)
    got = model(data)
    assert sorted(got) == ["loss_box_reg", "loss_cls"]
    a, b = float(got["loss_box_reg"].detach()), total / norm
    print(f"\nloss_box_reg: hip {a:.7f} restated {b:.7f} ({npos} positives)")
    assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3)
    assert abs(float(model.loss_normalizer) - norm) < 1e-3
    # one positive with dw above the clamp log(1000 / 16) = 4.135
    first = torch.nonzero(pos.view(-1))[0, 0].item()
    n0, r0 = divmod(first, R)
    buf = box_buf.clone()
    buf[n0, r0 // A, (r0 % A) * 5 + 2] = 9.0
    pdel = buf.cpu()[..., : A * 5].reshape(N, R, 5)
    total, g64, boxes = _restated_box_loss(pdel, anchors.cpu(), matched.cpu(), pos, W5)
    assert abs(float(boxes[0, 2]) / float(anchors[r0, 2]) - 62.5) < 1e-3
    nrm = torch.tensor([norm], device=cuda)
    sums = HF.retina_riou_loss_fwd(buf, pitch, lab, anchors, matched, N, R, A, K, W5, model.scale_clamp, nrm.clone(), 0.9)
    print(f"clamped case: sum hip {float(sums[0]):.7f} restated {total:.7f}")
    assert float(sums[1]) == npos and abs(float(sums[0]) - total) <= 1e-4 * max(abs(total), 1e-3)
    g64 = g64 / norm
    near = torch.zeros_like(pos)
    near[pos] = RL.margin(boxes, matched.cpu().double()[pos]) < MARGIN
    overlap = torch.zeros_like(pos)
    overlap[pos] = RL.iou(boxes, matched.cpu().double()[pos]) > 0
    keep = pos & ~near & overlap
    print(f"{int(near.sum())} of {npos} positives inside the margin, {int((pos & ~overlap).sum())} without overlap")
    assert int(near.sum()) <= MAX_EXCLUDED * npos and int(keep.sum()) >= 10 and keep[n0, r0]
    for mode, row_bar, agg_bar in (("bf16", None, 4e-3), ("fp32", FUSED_ROW_BAR, FUSED_AGG_BAR)):
        prev = HF.set_precision(mode)
        try:
            d = torch.full((N, P, pitch), 7.0, dtype=HF.ACT_DTYPE, device=cuda)
            HF.retina_riou_loss_bwd(buf, pitch, lab, anchors, matched, N, R, A, K, W5, model.scale_clamp, torch.ones(1, device=cuda), nrm, d)
        finally:
            HF.set_precision(prev)
        gotd = d.double().cpu()[..., : A * 5].reshape(N, R, 5)
        e, r = (gotd - g64)[keep], g64[keep]
        agg = float(e.norm() / r.norm())
        row = float((e.norm(dim=1) / r.norm(dim=1)).max())
        print(f"{mode}: delta-gradient rows of {int(keep.sum())} positives off by {agg:.3g} of their norm together, worst row {row:.3g}")
        assert agg <= agg_bar, (mode, agg)
        assert row_bar is None or row <= row_bar, (mode, row)
        assert (gotd[~pos] == 0).all() and (d[..., A * 5:] == 0).all()
        assert gotd[n0, r0, 2] == 0 and g64[n0, r0, 2] == 0 and gotd[n0, r0].abs().sum() > 0
        assert (gotd[pos & ~overlap] == 0).all()


# ------------------------------------------------------------------------------------------------ 5. model
def _train_step(model, opt, data):
    losses = model(data)
    total = sum(losses.values())
    opt.zero_grad()
    model.arena.begin_backward(); total.backward(); model.arena.finish_backward()
    opt.step()
    return losses


def _one_step(box_loss):
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.solver import build_optimizer

    cfg = _cfg(box_loss)
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    opt = build_optimizer(cfg, model)
    losses = _train_step(model, opt, _data(2, 128, 160, 41, K8))
    return model, {k: v.detach().clone() for k, v in losses.items()}


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_training_step_with_rotated_iou(cuda, mode):
    """One training step of the R18 model with "rotated_iou" (bf16 product path and SOD_PRECISION=fp32 mode): both losses finite, every
    trainable parameter has a finite gradient, bbox_pred's real rows have a non-zero one and its pad rows an exactly zero one; the same
    seed with "smooth_l1" gives the same loss_cls bit for bit (the labels do not depend on the loss type) and another loss_box_reg."""
    from slenderobjdet_amd.layers import functional as HF

    prev = HF.set_precision(mode)
    try:
        model, losses = _one_step("rotated_iou")
        _, ref = _one_step("smooth_l1")
    finally:
        HF.set_precision(prev)
    vals = {k: float(v) for k, v in losses.items()}
    print(f"\n{mode}: rotated_iou {vals}, smooth_l1 { {k: float(v) for k, v in ref.items()} }")
    assert sorted(vals) == ["loss_box_reg", "loss_cls"] and all(math.isfinite(v) for v in vals.values())
    assert torch.equal(losses["loss_cls"], ref["loss_cls"])
    assert float(losses["loss_box_reg"]) != float(ref["loss_box_reg"]) and 0.0 < vals["loss_box_reg"]
    n = 0
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            n += 1
    assert n > 20
    A5 = model.head.num_anchors * 5
    gw = model.head.bbox_pred.weight.grad
    assert gw[:A5].abs().sum() > 0 and (gw[A5:] == 0).all() and (model.head.bbox_pred.bias.grad[A5:] == 0).all()
