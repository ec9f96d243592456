"""The Gaussian KL-divergence box loss ("rotated_kld") on the GPU against the float64 restatement of tests/rotated_kld_loss_restated.py
(covariance matrices, inv, logdet): the pair operator and layers.rotated_kld_loss, the special cases, the fused RetinaNet kernels on the
R18 model's own buffers, the row kernels in both row forms and bit for bit against the RetinaNet kernels, and training steps of
RotatedRetinaNet and of the small rotated R-CNN.  The model, the data and the buffers are those of tests/test_gpu_rotated_iou_loss.py
and tests/test_gpu_rcnn_box_loss.py.

The loss has no kinks, so NOTHING is excluded: every generated pair, positive and row is asserted.  Two figures per test: the worst
|L - L64| (for a fused sum: |sum - sum64| / number of terms) and the worst gradient row error over the row's float64 norm
(KL.row_errors; a row whose exact gradient is zero counts by its absolute error).  The bars are FOUR TIMES the values measured on an
MI355X, per test; the measured values are in MEASURED and in the docstrings, and every run prints its own."""
import functools
import math

import pytest
import torch

import rcnn_box_loss_restated as RR
import rotated_kld_loss_restated as KL
import test_gpu_rotated_iou_loss as SIB

pytestmark = pytest.mark.gpu

K8, W5 = SIB.K8, SIB.W5
K3, W_ROI = 3, RR.W_ROI5
# (worst |L - L64|, worst gradient row) measured on an MI355X; a float32 emulation of the closed form on a CPU gave 3e-7 and 1.6e-6.
# "rows" stands an order of magnitude above the pairs, and the cause is the INPUT of the loss, not its arithmetic: a row's box is decoded in
# float32 by Box2BoxTransformRotated.apply_deltas, whose angle wrap fmodf(a + 180, 360) - 180 leaves the angle on the float32 grid near
# 190 degrees (steps of 1.5e-5 degrees), and the worst row (foreground row 83: decoded angle 10.78238, gt 11.12581) misses its gt's angle
# by 0.34 degrees - 7e-6 of 0.34 is 2e-5 of the angle gradient, which dominates the row of a slender box.  Reproduced on a CPU: a float32
# emulation of decode, closed form and chain gives 1.39e-5 on that row, and FLOAT64 arithmetic on the float32-decoded boxes 1.37e-5, all
# of it in the angle's column.  The pairs, whose float32 boxes ARE the inputs, meet the expectation.
MEASURED = {"pair": (2.59e-7, 1.96e-6), "special": (1.23e-7, 8.32e-7), "fused": (1.11e-8, 6.27e-7), "rows": (7.53e-8, 1.40e-5), "step": (5.71e-8, None)}
BAR = {k: tuple(None if x is None else 4 * x for x in v) for k, v in MEASURED.items()}
# a gradient stored as bf16 (8 significant bits): every element within half an ulp, 2^-8 of itself, so a row within 2^-8 of its norm -
# from the format, not from a measurement (measured: worst row 3.16e-3, all rows together 1.84e-3)
BF16_ROW = 2.0 ** -8


def _call(fn, *tensors):
    return fn(*[t.contiguous() for t in tensors])


# ------------------------------------------------------------------------------------------------ 1. pairs
@functools.lru_cache(maxsize=None)
def _pair_case():
    """1 024 near pairs then 1 024 far pairs and their float64 loss and gradient (computed once, shared, never modified)."""
    pred, gt = KL.pairs(1024, 1024)
    assert float(pred[:, 2:4].min()) > 0 and float(gt[:, 2:4].min()) > 0          # the generators floor w and h at 1: no seed to avoid
    ref_l, ref_g = KL.loss_and_grad(pred, gt)
    return pred, gt, ref_l, ref_g


def test_pairs_forward_and_backward_vs_float64(cuda):
    """1 024 near + 1 024 far pairs, every one asserted.  Measured on an MI355X: worst |L - L64| 2.59e-7 (far half 1.95e-7), worst
    gradient row 1.96e-6 of its norm (a far pair), all rows together |e| / |ref| = 2.21e-7; sum_out 7.4e-8 relative.  P = 1, 255, 257 and 1 024 are prefixes of the near pairs and give the rows of the big call bit for
    bit (one pair per lane: no row depends on another); sum_out within the float32 summation's reach of the elements' sum; P = 0 gives sum
    0 and raises nothing.  grad_scale is linear (0.25 gives exactly a quarter); layers.rotated_kld_loss under autograd ("sum", "mean",
    "none") returns the same numbers."""
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.layers import rotated_kld_loss

    pred, gt, ref_l, ref_g = _pair_case()
    a, b = pred.float().to(cuda), gt.float().to(cuda)
    elem, s = HF.rotated_kld_loss_fwd(a, b)
    d = HF.rotated_kld_loss_bwd(a, b)
    err_l, row, agg = KL.row_errors(elem.cpu(), d.cpu(), ref_l, ref_g)
    far_l, far_row, _ = KL.row_errors(elem.cpu()[1024:], d.cpu()[1024:], ref_l[1024:], ref_g[1024:])
    want = float(elem.double().sum())
    rel = abs(float(s) - want) / want
    print(f"\npairs: {elem.numel()} pairs, worst |L - L64| {err_l:.3g} (far half {far_l:.3g}), worst gradient row {row:.3g} of its norm (far half "
          f"{far_row:.3g}), all rows |e| / |ref| = {agg:.3g}; sum {float(s):.7f} against {want:.7f} (rel {rel:.3g}); bars {BAR['pair']}")
    assert elem.shape == (2048,) and d.shape == (2048, 5)
    assert bool(torch.isfinite(elem).all()) and bool((elem >= 0).all()) and bool((elem < 1).all()) and bool(torch.isfinite(d).all())
    assert err_l <= BAR["pair"][0] and row <= BAR["pair"][1]
    assert rel <= 1e-6
    for P in (1, 255, 257, 1024):
        e2, s2 = _call(HF.rotated_kld_loss_fwd, a[:P], b[:P])
        d2 = _call(HF.rotated_kld_loss_bwd, a[:P], b[:P])
        w2 = float(elem[:P].double().sum())
        assert torch.equal(e2, elem[:P]) and torch.equal(d2, d[:P]) and abs(float(s2) - w2) <= 1e-6 * w2, P
    ef, _ = _call(HF.rotated_kld_loss_fwd, a[1024:], b[1024:])
    assert torch.equal(ef, elem[1024:]) and torch.equal(_call(HF.rotated_kld_loss_bwd, a[1024:], b[1024:]), d[1024:])
    e0, s0 = _call(HF.rotated_kld_loss_fwd, a[:0], b[:0])
    d0 = _call(HF.rotated_kld_loss_bwd, a[:0], b[:0])
    assert e0.numel() == 0 and float(s0) == 0.0 and d0.shape == (0, 5)
    d1 = HF.rotated_kld_loss_bwd(a, b, grad_scale=torch.ones(1, device=cuda))
    dq = HF.rotated_kld_loss_bwd(a, b, grad_scale=torch.full((1,), 0.25, device=cuda))
    assert torch.equal(d1, d) and torch.equal(dq, d * 0.25)
    for reduction in ("sum", "mean", "none"):
        ar = a.clone().requires_grad_(True)
        l = rotated_kld_loss(ar, b, reduction=reduction)
        if reduction == "none":
            assert torch.equal(l, elem)
            l.sum().backward()
            assert torch.equal(ar.grad, d)
        else:
            n = a.shape[0] if reduction == "mean" else 1
            assert abs(float(l.detach()) - want / n) <= 1e-6 * want / n
            (l * 2.0).backward()
            assert float((ar.grad - d * (2.0 / n)).abs().max()) <= 1e-6 * (2.0 / n) * float(d.abs().max())
    z0 = rotated_kld_loss(a[:0].clone().requires_grad_(True), b[:0], reduction="mean")
    assert float(z0.detach()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. special cases
def test_special_cases(cuda):
    """Identical boxes; one box written as (h, w, t + 90), t + 180 and t - 180; squares with 0 and 45 degrees of angle error; the ratios
    1, 2, 5, 10, 50 with 3 degrees of angle error; the sliver pair.  All but the sliver against the float64 restatement - measured on an
    MI355X: worst |L - L64| 1.23e-7, worst gradient row 8.32e-7 (rows whose exact gradient is zero - the first five - count by their
    absolute error); the first six losses came out exactly 0, dL / d angle 0, 0.002034, 0.019165, 0.062175, 0.08337 per degree as in
    float64, the sliver 0.97016579 (|e| 9.1e-9).  The loss of the first five is within the bar of 0, and so is the angle gradient of
    both squares (the square with 45 degrees of error: exactly 0, its loss 0 - an isotropic Gaussian has no angle).  dL / d angle of the
    kernel's own output is 0 at ratio 1 and strictly increasing after it.  The sliver (gt 8000 x 1.5e-5 px): finite, in [0, 1), within the
    bar of 0.97016578 (the matrix definition at 50 digits; float64 matrices cannot hold that covariance), its gradient finite.  A zero
    side gives NaN."""
    from slenderobjdet_amd.layers import functional as HF

    pred, gt, names = KL.special_cases()
    a, b = pred.float().to(cuda), gt.float().to(cuda)
    elem, _ = HF.rotated_kld_loss_fwd(a, b)
    d = HF.rotated_kld_loss_bwd(a, b)
    el, dg = elem.cpu(), d.cpu()
    i = names.index("sliver")
    keep = torch.arange(len(names)) != i
    ref_l, ref_g = KL.loss_and_grad(pred[keep], gt[keep])
    err_l, row, _ = KL.row_errors(el[keep], dg[keep], ref_l, ref_g)
    sl = float(el[i])
    ratios = [float(dg[names.index(f"ratio_{r}"), 4]) for r in KL.RATIOS]
    print(f"\nspecial cases: worst |L - L64| {err_l:.3g}, worst gradient row {row:.3g}; losses { {n: float(v) for n, v in zip(names, el)} }; "
          f"dL / d angle at ratios {KL.RATIOS}: {[round(v, 6) for v in ratios]} (float64 {[round(float(v), 6) for v in ref_g[6:11, 4]]}); sliver {sl:.8f} "
          f"(|e| {abs(sl - KL.SLIVER_LOSS):.3g}), its gradient {dg[i].tolist()}; bars {BAR['special']}")
    assert bool(torch.isfinite(el).all()) and bool(torch.isfinite(dg).all()) and bool((el >= 0).all()) and bool((el < 1).all())
    assert err_l <= BAR["special"][0] and row <= BAR["special"][1]
    zero = [names.index(n) for n in ("identical", "swapped_90", "plus_180", "minus_180", "square_0", "square_45")]
    assert float(el[zero].abs().max()) <= BAR["special"][0] and float(ref_l[:6].abs().max()) <= 1e-12
    assert float(dg[zero[:5]].norm(dim=1).max()) <= BAR["special"][1]
    assert float(dg[zero[4:], 4].abs().max()) <= BAR["special"][1] and float(dg[names.index("square_45"), 4]) == 0.0
    assert ratios[0] == 0.0 and all(y > x for x, y in zip(ratios, ratios[1:]))
    assert 0.0 <= sl < 1.0 and abs(sl - KL.SLIVER_LOSS) <= BAR["special"][0]
    bad = b[:1].clone()
    bad[0, 3] = 0.0
    e_bad, _ = HF.rotated_kld_loss_fwd(a[:1].contiguous(), bad)
    assert bool(torch.isnan(e_bad).all()) and bool(torch.isnan(HF.rotated_kld_loss_bwd(bad, a[:1].contiguous())).all())


# ------------------------------------------------------------------------------------------------ 3. fused RetinaNet kernels
def test_fused_retina_kernels_vs_restatement(cuda):
    """sod_retina_rkld_loss_* on the R18 model's own prediction buffer, labels and matched boxes (2 images of 128 x 160, A = 6, K = 8,
    pitch 32, data seed 21), one positive's dw pushed above the clamp.  sums[0] against the float64 restatement chained through float64
    apply_deltas, per positive; sums[1] the number of positives; the EMA normaliser 0.9 * 100 + 0.1 * max(npos, 1) within float32
    rounding.  dpred pre-filled with NaN comes back with EVERY element written: the positives' rows against float64 autograd w.r.t. the
    deltas - fp32 storage within the measured bar, bf16 storage within that plus 2^-8 (half an ulp of bf16) -, exact zeros in the rows of
    non-positives and in the pad columns.  The clamped dw has gradient exactly 0 while its row is not zero.  Measured on an MI355X:
    sum 34.0006256 against 34.0006263 over 63 positives (|e| / npos 1.11e-8), worst fp32 row 6.27e-7 of its norm (all rows together
    2.43e-7), worst bf16 row 3.16e-3 (all rows together 1.84e-3)."""
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.modeling import build_model

    cfg = SIB._cfg("rotated_kld")
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    A, K, pitch = model.head.num_anchors, model.num_classes, model.head.box_pitch
    assert (A, K, pitch) == (6, K8, 32)
    data = SIB._data(2, 128, 160, 21, K)
    _, hw, _, box_buf, _ = SIB._buffers(model, data)
    anchors = model.anchors_for(hw)
    lab, matched = model.label_anchors(anchors, [x["instances"] for x in data])
    N, P = box_buf.shape[:2]
    R = P * A
    assert matched.shape == (N, R, 5)
    pos = ((lab >= 0) & (lab != K)).cpu()
    npos = int(pos.sum())
    assert npos >= 10 and int((~pos).sum()) > 0
    first = torch.nonzero(pos.view(-1))[0, 0].item()
    n0, r0 = divmod(first, R)
    buf = box_buf.clone()
    buf[n0, r0 // A, (r0 % A) * 5 + 2] = 9.0          # dw above the clamp log(1000 / 16) = 4.135
    pdel = buf.cpu()[..., : A * 5].reshape(N, R, 5)
    total, g64, boxes = KL.restated_sum(pdel, anchors.cpu(), matched.cpu(), pos, W5)
    assert abs(float(boxes[0, 2]) / float(anchors[r0, 2]) - 62.5) < 1e-3
    nrm = torch.full((1,), 100.0, device=cuda)
    sums = HF.retina_rkld_loss_fwd(buf, pitch, lab, anchors, matched, N, R, A, K, W5, model.scale_clamp, nrm, 0.9)
    norm = 0.9 * 100.0 + 0.1 * max(npos, 1)
    err_s = abs(float(sums[0]) - total) / npos
    print(f"\nfused: sum hip {float(sums[0]):.7f} restated {total:.7f} ({npos} positives, |e| / npos {err_s:.3g}), normaliser {float(nrm):.6f} ({norm:.6f})")
    g64 = g64 / norm
    figures = {}
    for mode in ("bf16", "fp32"):
        prev = HF.set_precision(mode)
        try:
            d = torch.full((N, P, pitch), float("nan"), dtype=HF.ACT_DTYPE, device=cuda)
            HF.retina_rkld_loss_bwd(buf, pitch, lab, anchors, matched, N, R, A, K, W5, model.scale_clamp, torch.ones(1, device=cuda), nrm, d)
        finally:
            HF.set_precision(prev)
        assert bool(torch.isfinite(d.float()).all()), mode          # every element written
        gotd = d.double().cpu()[..., : A * 5].reshape(N, R, 5)
        _, row, agg = KL.row_errors(None, gotd[pos], None, g64[pos])
        figures[mode] = row
        print(f"{mode}: delta-gradient rows of {npos} positives: worst row {row:.3g} of its norm, all rows |e| / |ref| = {agg:.3g}")
        assert (gotd[~pos] == 0).all() and (d[..., A * 5:] == 0).all()
        assert gotd[n0, r0, 2] == 0 and g64[n0, r0, 2] == 0 and gotd[n0, r0].abs().sum() > 0
    print(f"bars {BAR['fused']}, bf16 rows {BAR['fused'][1] + BF16_ROW:.3g}")
    assert float(sums[1]) == npos and err_s <= BAR["fused"][0]
    assert abs(float(nrm) - norm) <= 1e-5 * norm
    assert figures["fp32"] <= BAR["fused"][1] and figures["bf16"] <= BAR["fused"][1] + BF16_ROW


# ------------------------------------------------------------------------------------------------ 4. row kernels
@functools.lru_cache(maxsize=None)
def _rows_case():
    """300 rows from the recipe of tests/rcnn_box_loss_restated.py (150 near + 150 far; K = 3, ld = K * 5 + 1 = 16; every 7th row
    background, label K), every 11th row ignored (label -1); the RPN form of the same numbers: the rows' own five columns, int8 labels
    1 (foreground), 0 and -1.  -> both forms with their float64 sums and gradients (computed once, shared, never modified)."""
    pred, labels, src, gt = RR.rotated_rows(150, 150, K3)
    labels = labels.clone()
    labels[4::11] = -1
    R, ld = pred.shape
    assert (R, ld) == (300, K3 * 5 + 1) and set(labels.tolist()) == {-1, 0, 1, 2, 3}
    fg = (labels >= 0) & (labels < K3)
    cols = (labels.long().clamp(0, K3 - 1))[:, None] * 5 + torch.arange(5)[None]
    rows5 = torch.gather(pred, 1, cols).contiguous()
    lab8 = torch.where(fg, 1, torch.where(torch.arange(R) % 2 == 0, 0, -1)).to(torch.int8)
    assert set(lab8.tolist()) == {-1, 0, 1}
    forms = {"frcnn": (pred, labels, K3), "rpn": (rows5, lab8, 1)}
    refs = {f: KL.rows_loss(f, p, l, k, src, gt, W_ROI) for f, (p, l, k) in forms.items()}
    assert torch.equal(refs["frcnn"][2], fg) and torch.equal(refs["rpn"][2], fg)
    return forms, refs, src, gt, fg, cols


@pytest.mark.parametrize("R", [0, 1, 300])
@pytest.mark.parametrize("form", ["frcnn", "rpn"])
def test_rows_vs_float64(cuda, form, R):
    """Both row forms at R = 0, 1 and 300 (prefixes of one set of rows).  Forward sum against float64, per foreground row; backward with
    grad_scale 0.5 on the device and scale_mul 1 / 300 into a buffer that held NaN: EVERY element written, every foreground row against
    float64 autograd, exact zeros in non-foreground rows (labels -1 and K; 0 and -1), in the other classes' columns and in the pad
    column.  Two calls give the same bits; R = 0 gives sum 0 and writes nothing.  Measured on an MI355X over the cases: |sum - sum64| / rows
    7.53e-8 (R = 1; R = 300: 131.8901825 against 131.8901813 over 235 foreground rows, 5.1e-9), worst row 1.40e-5 of its norm (R = 300,
    all rows together 1.88e-6; R = 1: 3.05e-7) - the float32 decode's angle grid against an angle error of a degree: see MEASURED."""
    from slenderobjdet_amd.layers import functional as HF

    forms, _, src, gt, _, _ = _rows_case()
    pred, labels, K = forms[form]
    pred, labels, src, gt = pred[:R].contiguous(), labels[:R].contiguous(), src[:R].contiguous(), gt[:R].contiguous()
    total, g64, fg, boxes = KL.rows_loss(form, pred, labels, K, src, gt, W_ROI)
    ld = pred.shape[1]
    p, l, s, g = pred.to(cuda), labels.to(cuda), src.to(cuda), gt.to(cuda)
    got_s = HF.rows_box_loss_fwd("rotated_kld", form, p, l, K, s, g, W_ROI, RR.SCALE_CLAMP)
    again = HF.rows_box_loss_fwd("rotated_kld", form, p, l, K, s, g, W_ROI, RR.SCALE_CLAMP)
    half = torch.full((1,), 0.5, device=cuda)
    d = torch.full((R, ld), float("nan"), device=cuda)
    ret = HF.rows_box_loss_bwd("rotated_kld", form, p, l, K, s, g, W_ROI, RR.SCALE_CLAMP, half, 1.0 / 300, out=d)
    d2 = HF.rows_box_loss_bwd("rotated_kld", form, p, l, K, s, g, W_ROI, RR.SCALE_CLAMP, half, 1.0 / 300)
    assert ret is d and got_s.shape == (1,) and torch.equal(got_s, again) and d2.shape == (R, ld)
    nfg = int(fg.sum())
    if R == 0:
        assert float(got_s) == 0.0 and total == 0.0
        return
    assert bool(torch.isfinite(d).all()) and torch.equal(d, d2)          # every element written
    got, ref = d.cpu().double(), g64 * (0.5 / 300)
    err_s = abs(float(got_s) - total) / max(nfg, 1)
    _, row, agg = KL.row_errors(None, got[fg], None, ref[fg])
    rows_e = ((got - ref)[fg].norm(dim=1) / ref[fg].norm(dim=1))
    w = int(rows_e.argmax())
    print(f"\nrows {form} R = {R}: {nfg} foreground rows, sum hip {float(got_s):.7f} float64 {total:.7f} (|e| / rows {err_s:.3g}), worst row {row:.3g} "
          f"of its norm (decoded box {[round(float(x), 4) for x in boxes[w]]}, gt {[round(float(x), 4) for x in gt[fg][w]]}), "
          f"all rows |e| / |ref| = {agg:.3g}; bars {BAR['rows']}")
    assert nfg >= 1 and (R == 1 or nfg > 200)
    own = torch.zeros(R, ld, dtype=torch.bool)
    c0 = labels.long()[fg] * 5 if form == "frcnn" else torch.zeros(nfg, dtype=torch.long)
    own[fg] = own[fg].scatter(1, c0[:, None] + torch.arange(5)[None], torch.ones(nfg, 5, dtype=torch.bool))
    assert (got[~own] == 0).all() and (ref[~own] == 0).all() and (got[~fg] == 0).all()
    assert err_s <= BAR["rows"][0] and row <= BAR["rows"][1]


def test_rows_equal_the_retina_kernels_bit_for_bit(cuda):
    """The same numbers as RPN rows (int8 labels, ld = 5), as a RetinaNet buffer (N = 1, A = 1, pitch = 5; label 1 -> class 0, everything
    else -> num_classes) and as Fast R-CNN rows: all three call one definition of the policy, so with both scales 1 the delta gradients
    are torch.equal (fp32 storage), and the sums - the kernels add the blocks' partial sums in the same fixed order - are torch.equal
    too.  The check of tests/test_gpu_rcnn_box_loss.py, made for the new kind."""
    from slenderobjdet_amd.layers import functional as HF

    forms, _, src, gt, fg, cols = _rows_case()
    (pred, labels, _), (rows5, lab8, _) = forms["frcnn"], forms["rpn"]
    R = rows5.shape[0]
    lab32 = torch.where(fg, 0, 1).to(torch.int32)
    p, s, g = rows5.to(cuda), src.to(cuda), gt.to(cuda)
    one = torch.ones(1, device=cuda)
    s_rows = HF.rows_box_loss_fwd("rotated_kld", "rpn", p, lab8.to(cuda), 1, s, g, W_ROI, RR.SCALE_CLAMP)
    d_rows = torch.full((R, 5), 7.0, device=cuda)
    HF.rows_box_loss_bwd("rotated_kld", "rpn", p, lab8.to(cuda), 1, s, g, W_ROI, RR.SCALE_CLAMP, one, 1.0, out=d_rows)
    prev = HF.set_precision("fp32")
    try:
        sums = HF.retina_rkld_loss_fwd(p.view(1, R, 5), 5, lab32.to(cuda).view(1, R), s, g.view(1, R, 5), 1, R, 1, 1, W_ROI, RR.SCALE_CLAMP, one.clone(), 0.9)
        d_ret = torch.full((1, R, 5), 7.0, dtype=HF.ACT_DTYPE, device=cuda)
        assert d_ret.dtype == torch.float32
        HF.retina_rkld_loss_bwd(p.view(1, R, 5), 5, lab32.to(cuda).view(1, R), s, g.view(1, R, 5), 1, R, 1, 1, W_ROI, RR.SCALE_CLAMP, one, one, d_ret)
    finally:
        HF.set_precision(prev)
    s_frcnn = HF.rows_box_loss_fwd("rotated_kld", "frcnn", pred.to(cuda), labels.to(cuda), K3, s, g, W_ROI, RR.SCALE_CLAMP)
    d_frcnn = HF.rows_box_loss_bwd("rotated_kld", "frcnn", pred.to(cuda), labels.to(cuda), K3, s, g, W_ROI, RR.SCALE_CLAMP, one, 1.0)
    print(f"\nrows sum {float(s_rows):.7f}, retina sum {float(sums[0]):.7f}, Fast R-CNN rows sum {float(s_frcnn):.7f}, {int(sums[1])} positives")
    assert int(sums[1]) == int(fg.sum())
    assert torch.equal(s_rows, sums[:1]) and torch.equal(s_frcnn, s_rows)
    assert torch.equal(d_rows, d_ret.view(R, 5))
    assert (d_rows[~fg.to(cuda)] == 0).all() and d_rows[fg.to(cuda)].abs().sum() > 0
    assert torch.equal(torch.gather(d_frcnn, 1, cols.to(cuda))[fg.to(cuda)], d_rows[fg.to(cuda)])


# ------------------------------------------------------------------------------------------------ 5. training steps
def _finite_grads(model, at_least):
    n = 0
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            n += 1
    assert n > at_least


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_training_step_of_rotated_retinanet(cuda, mode):
    """One training step of the R18 RotatedRetinaNet with "rotated_kld" (bf16 product path and SOD_PRECISION=fp32 mode; 2 images of
    128 x 160, data seed 41): both losses finite, every trainable parameter has a finite gradient, bbox_pred's real rows a non-zero one and
    its pad rows an exactly zero one.  loss_box_reg equals the float64 restatement summed over the labels the model produced - on the
    model's own prediction buffer - divided by the normaliser the model used, per positive within the bar (measured on an MI355X:
    bf16 0.3668706 against 0.3668706 over 61 positives, 8.4e-9 per positive; fp32 mode 0.3672318 against 0.3672317, 2.3e-8; the bar is
    four times the worst of the four step tests, 5.71e-8).  The same seed with "smooth_l1" gives the same loss_cls bit for bit: the labels do not depend on the loss type."""
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.solver import build_optimizer

    prev = HF.set_precision(mode)
    try:
        cfg = SIB._cfg("rotated_kld")
        torch.manual_seed(0)
        model = build_model(cfg)
        model.train()
        opt = build_optimizer(cfg, model)
        data = SIB._data(2, 128, 160, 41, K8)
        A, K = model.head.num_anchors, model.num_classes
        _, hw, _, box_buf, _ = SIB._buffers(model, data)
        anchors = model.anchors_for(hw)
        lab, matched = model.label_anchors(anchors, [x["instances"] for x in data])
        losses = SIB._train_step(model, opt, data)
        torch.cuda.synchronize()
        _, ref = SIB._one_step("smooth_l1")
    finally:
        HF.set_precision(prev)
    N, P = box_buf.shape[:2]
    pos = ((lab >= 0) & (lab != K)).cpu()
    npos = int(pos.sum())
    total, _, _ = KL.restated_sum(box_buf.cpu()[..., : A * 5].reshape(N, P * A, 5), anchors.cpu(), matched.cpu(), pos, W5)
    norm = float(model.loss_normalizer)
    got = float(losses["loss_box_reg"].detach())
    err = abs(got * norm - total) / npos
    vals = {k: float(v) for k, v in losses.items()}
    print(f"\n{mode}: {vals}; loss_box_reg hip {got:.7f} restated {total / norm:.7f} ({npos} positives, normaliser {norm:.4f}, |e| per positive {err:.3g}; "
          f"bar {BAR['step'][0]:.3g}); smooth_l1 { {k: float(v) for k, v in ref.items()} }")
    assert sorted(vals) == ["loss_box_reg", "loss_cls"] and all(math.isfinite(v) for v in vals.values())
    assert npos >= 10 and abs(norm - (0.9 * 100.0 + 0.1 * npos)) <= 1e-3
    assert err <= BAR["step"][0]
    assert torch.equal(losses["loss_cls"].detach(), ref["loss_cls"]) and 0.0 < got != float(ref["loss_box_reg"])
    _finite_grads(model, 20)
    A5 = A * 5
    gw = model.head.bbox_pred.weight.grad
    assert gw[:A5].abs().sum() > 0 and (gw[A5:] == 0).all() and (model.head.bbox_pred.bias.grad[A5:] == 0).all()


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_training_step_of_the_rotated_rcnn(cuda, mode):
    """One step of the small rotated two-stage model of tests/test_gpu_rcnn.py (2 images of 96 x 128, data seed 21) with "rotated_kld" on
    both stages, the residual branches damped as tests/test_gpu_rcnn_box_loss.py damps them so that the runs are comparable (the loss
    itself does not need it: see DESIGN.md).  All four losses finite, every trainable parameter has a finite gradient, the real rows of
    bbox_pred's and of the RPN's anchor_deltas' weight gradient non-zero and the pad rows exactly zero.  The box predictor's deltas on
    ``roi_heads.last_proposals`` and the RPN head's deltas gathered at ``RPN.last_sampled`` - the numbers the kernels read - go through
    the float64 restatement: loss_box_reg = sum / number of sampled rows, loss_rpn_loc = sum / (BATCH_SIZE_PER_IMAGE * N), per
    foreground row within the bar (measured on an MI355X: bf16 loss_box_reg 0.0062726 over 8 foreground rows of 32, 2.0e-8 per row,
    loss_rpn_loc 0.0317604 over 16 positives of 128, 1.7e-9; fp32 mode 0.0062393, 5.71e-8 and 0.0316588, 2.6e-8)."""
    import test_gpu_rcnn_box_loss as RB

    model, got, cap = RB._step_with(True, "rotated_kld", mode, cuda)
    assert set(got) == {"loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg"}
    rpn, roi = model.proposal_generator, model.roi_heads
    assert rpn.box_reg_loss_type == roi.box_predictor.box_reg_loss_type == "rotated_kld"
    props = roi.last_proposals
    R = sum(len(p) for p in props)
    deltas = cap["roi"].view(R, -1).cpu()
    cls = torch.cat([p.gt_classes for p in props]).to(torch.int32).cpu()
    boxes = torch.cat([p.proposal_boxes.tensor for p in props]).cpu()
    gtb = torch.cat([p.gt_boxes.tensor for p in props]).cpu()
    total, _, fg, _ = KL.rows_loss("frcnn", deltas, cls, 80, boxes, gtb, roi.box_predictor.box2box_transform.weights)
    idx, labels_s, (src_s, gt_s) = rpn.last_sampled
    A, N, S = rpn.head.num_anchors, idx.shape[0], rpn.batch_size_per_image
    flat = torch.cat([x[..., :A * 5].reshape(N, -1, 5) for x in cap["rpn"]], 1)
    rows = torch.gather(flat, 1, idx.clamp(min=0).long()[:, :, None].expand(-1, -1, 5)).reshape(-1, 5).cpu()
    total_r, _, fg_r, _ = KL.rows_loss("rpn", rows, labels_s.view(-1).cpu(), 1, src_s.reshape(-1, 5).cpu(), gt_s.reshape(-1, 5).cpu(),
                                       rpn.box2box_transform.weights)
    a_box, a_loc = float(got["loss_box_reg"].detach()), float(got["loss_rpn_loc"].detach())
    nfg, nfg_r = int(fg.sum()), int(fg_r.sum())
    e_box = abs(a_box * R - total) / max(nfg, 1)
    e_loc = abs(a_loc * (S * N) / rpn.loss_weight["loss_rpn_loc"] - total_r) / max(nfg_r, 1)
    print(f"\nrotated_kld {mode}: { {k: float(v) for k, v in got.items()} }; loss_box_reg hip {a_box:.7f} restated {total / R:.7f} ({nfg} of {R} rows "
          f"foreground, |e| per row {e_box:.3g}); loss_rpn_loc hip {a_loc:.7f} restated {total_r / (S * N):.7f} ({nfg_r} of {S * N} sampled anchors "
          f"positive, |e| per row {e_loc:.3g}); bar {BAR['step'][0]:.3g}")
    assert all(math.isfinite(float(v)) for v in got.values()), got
    assert nfg >= 2 and nfg_r >= 2
    assert e_box <= BAR["step"][0] and e_loc <= BAR["step"][0]
    _finite_grads(model, 30)
    gw = roi.box_predictor.bbox_pred.weight.grad
    assert gw.shape[0] == roi.box_predictor.box_out and gw[:80 * 5].abs().sum() > 0 and (gw[80 * 5:] == 0).all()
    ga = rpn.head.anchor_deltas.conv.weight.grad
    assert ga.shape[0] == rpn.head.delta_pad > A * 5 and ga[:A * 5].abs().sum() > 0 and (ga[A * 5:] == 0).all()
