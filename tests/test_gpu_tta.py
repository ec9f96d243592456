"""Test-time augmentation on the GPU: the merge kernel (csrc/tta.hip) and the wrapper (modeling/test_time_augmentation.py) against the
numpy float64 restatement (tests/tta_restated.py).

Tolerances.  A merged coordinate is one or two float32 operations on a value bounded by max(H, W, h_a, w_a): the un-flip's subtraction,
the product with the scale, and the scale's own rounding from double.  Each is a relative 2^-24; the bound used throughout is
4 * 2^-22 * max(H, W, h_a, w_a).  NMS decisions are compared exactly, after the test has asserted in float64 that every same-class pair
of candidates is further from the threshold than the float32 IoU of class-shifted boxes can move it."""
import math

import numpy as np
import pytest
import torch

import tta_restated as R

pytestmark = pytest.mark.gpu

NEG_INF = -math.inf


def _tol(*sides):
    return 4 * 2.0 ** -22 * max(sides)


def _merge(cuda, runs, out_sizes, A, D, thresh=1e-8):
    """runs: [(image, slot, boxes (n, 4), scores (n), classes (n), (h_a, w_a), flip)] of numpy arrays -> HF.tta_merge_candidates."""
    from slenderobjdet_amd.layers import functional as HF

    off = [0]
    for r in runs:
        off.append(off[-1] + len(r[3]))
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(r[k], dtype=dt).reshape((-1, 4) if k == 2 else (-1,)) for r in runs])).to(cuda)
    table = [(r[0], r[1], r[5][0], r[5][1], r[6]) for r in runs]
    return HF.tta_merge_candidates(cat(2, np.float32), cat(3, np.float32), cat(4, np.int32), off, table, out_sizes, A, D, thresh)


def _rand_boxes(rng, n, h, w):
    x = np.sort(rng.uniform(0, w, (n, 2)), axis=1)
    y = np.sort(rng.uniform(0, h, (n, 2)), axis=1)
    return np.stack((x[:, 0], y[:, 0], x[:, 1], y[:, 1]), 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. the merge kernel
def test_merge_kernel_matches_restatement(cuda):
    from slenderobjdet_amd import _C

    rng = np.random.RandomState(0)
    out_sizes = [(37, 53), (64, 48)]
    A, D = 3, 8
    geo = [(0, 0, (50, 71), False, 8), (0, 1, (61, 87), True, 3), (0, 2, (29, 41), False, 0),
           (1, 0, (75, 56), True, 3), (1, 1, (90, 67), False, 8), (1, 2, (40, 30), False, 0)]
    runs = []
    for b, a, (ha, wa), flip, n in geo:
        boxes = _rand_boxes(rng, n, ha, wa)
        scores = rng.uniform(0.05, 1.0, n).astype(np.float32)
        classes = rng.randint(0, 2, n).astype(np.int32)
        if n == 8:
            boxes[1, 2] = np.nan
            scores[2] = np.inf
            scores[3], scores[4] = 1e-8, 5e-9
            boxes[5] = (wa - 9.5, ha - 7.25, wa + 10.0, ha + 6.0)          # leaves the image to the right and below
            classes[6], classes[7] = 0, 1
        runs.append((b, a, boxes, scores, classes, (ha, wa), flip))
    # every branch is present in the inputs
    assert sorted({len(r[3]) for r in runs}) == [0, 3, 8]
    assert any(np.isnan(r[2]).any() for r in runs) and any(np.isinf(r[3]).any() for r in runs)
    assert any((r[3] == np.float32(1e-8)).any() for r in runs) and any((r[3] == np.float32(5e-9)).any() for r in runs)
    assert any(((r[2][:, 2] > r[5][1]) & (r[2][:, 3] > r[5][0])).any() for r in runs)
    assert {int(c) for r in runs for c in r[4]} == {0, 1}
    assert {b for b, *_ in geo if any(g[0] == b and g[3] for g in geo)} == {0, 1}          # one flipped run per image

    gb, gs, gc = (t.cpu().numpy() for t in _merge(cuda, runs, out_sizes, A, D))
    assert gb.shape == (2, A * D, 4) and gs.shape == (2, A * D) and gc.shape == (2, A * D) and gc.dtype == np.int32
    n_valid = n_empty = 0
    for b, a, boxes, scores, classes, aug, flip in runs:
        H, W = out_sizes[b]
        eb, es, ec, valid = R.unmap(boxes, scores, classes, aug, flip, (H, W), 1e-8)
        for d in range(D):
            slot = a * D + d
            if d < len(scores) and valid[d]:
                n_valid += 1
                assert gs[b, slot] == scores[d] and gc[b, slot] == classes[d]
                assert np.abs(gb[b, slot] - eb[d]).max() <= _tol(H, W, *aug), (b, slot, gb[b, slot], eb[d])
                assert 0 <= gb[b, slot, 0] <= gb[b, slot, 2] <= W and 0 <= gb[b, slot, 1] <= gb[b, slot, 3] <= H
            else:
                n_empty += 1
                assert gs[b, slot] == NEG_INF and gc[b, slot] == 0 and (gb[b, slot] == 0).all(), (b, slot)
    assert n_valid == 2 * (3 + 8 - 4) and n_empty == 2 * A * D - n_valid
    # the clipped box sits on the right and bottom borders
    assert gb[0, 5, 2] == 53 and gb[0, 5, 3] == 37 and gb[1, D + 5, 2] == 48 and gb[1, D + 5, 3] == 64

    # a run with more detections than slots is an argument error, not a read past the slots
    with pytest.raises(_C.SlenderHipError, match="SOD_EARG"):
        _merge(cuda, runs, out_sizes, A, 7)
    # no detection at all: every slot empty
    none = [(0, 0, np.zeros((0, 4)), np.zeros(0), np.zeros(0), (50, 71), False)]
    eb, es, ec = _merge(cuda, none, [(37, 53)], 2, 4)
    assert (es == NEG_INF).all() and (eb == 0).all() and (ec == 0).all() and es.shape == (1, 8)


# ------------------------------------------------------------------------------------------------ 2. merge + NMS decisions
OUT_HW = (64, 96)
AUGS = [((64, 96), False), ((48, 72), True), ((80, 120), False)]


def _to_aug(box, aug, flip, out_hw=OUT_HW):
    """A box designed at the output size -> the augmented image's pixels (float64, rounded to float32 by the caller)."""
    (ha, wa), (H, W) = aug, out_hw
    x1, y1, x2, y2 = box
    x1, x2 = x1 * wa / W, x2 * wa / W
    if flip:
        x1, x2 = wa - x2, wa - x1
    return (x1, y1 * ha / H, x2, y2 * ha / H)


def _runs_from_design(design, augs=AUGS, out_hw=OUT_HW):
    """design: [(run, box at the output size, score, class)] -> [(0, a, boxes, scores, classes, aug, flip)] in run order."""
    runs = []
    for a, (aug, flip) in enumerate(augs):
        rows = [d for d in design if d[0] == a]
        boxes = np.array([_to_aug(d[1], aug, flip, out_hw) for d in rows], dtype=np.float32).reshape(-1, 4)
        runs.append((0, a, boxes, np.array([d[2] for d in rows], dtype=np.float32), np.array([d[3] for d in rows], dtype=np.int32), aug, flip))
    return runs


DESIGN_DECISIONS = [
    (0, (10, 10, 40, 40), 0.9, 0),           # kept
    (1, (11, 10, 41, 40), 0.8, 0),           # cross-augmentation duplicate of it (IoU 0.935): suppressed
    (2, (22, 10, 52, 40), 0.7, 0),           # near miss (IoU 0.43 / 0.46 with the two above): kept
    (1, (10, 10, 40, 40), 0.85, 1),          # same geometry, other class: kept
    (0, (60, 30, 90, 60), 0.6, 1),           # exact score tie between two augmentations ...
    (2, (61, 31, 91, 61), 0.6, 1),           # ... the earlier augmentation wins, this one (IoU 0.877) is suppressed
    (2, (60, 2, 90, 22), 0.3, 0),
]
_GRID = [(x, y, x + 20, y + 20) for y in (2, 34) for x in (2, 26, 50, 74)]
DESIGN_TOPK = [(i % 3, box, 0.95 - 0.05 * i, 0) for i, box in enumerate(_GRID)] + [(2, (3, 2, 23, 22), 0.2, 0), (1, (26, 35, 46, 55), 0.1, 0)]


@pytest.mark.parametrize("design,max_keep,n_expected", [(DESIGN_DECISIONS, 100, 5), (DESIGN_TOPK, 5, 5)])
def test_merge_then_nms_decisions(cuda, design, max_keep, n_expected):
    from slenderobjdet_amd.layers import functional as HF

    thr = 0.5
    runs = _runs_from_design(design)
    D = max(len(r[3]) for r in runs)
    rr = [(r[2], r[3], r[4], r[5], r[6]) for r in runs]
    cb, cs, cc, crun = R.merge_candidates(rr, OUT_HW, 1e-8)
    assert len(cb) == len(design) and (np.minimum(cb[:, 2] - cb[:, 0], cb[:, 3] - cb[:, 1]) >= 8).all()
    # EVERY same-class pair is at least 0.01 from the threshold (float64), and the intended kinds of pair are present
    assert R.same_class_iou_margin(cb, cc, thr) >= 0.01
    pairs = [(i, j) for i in range(len(cb)) for j in range(i + 1, len(cb))]
    assert any(cc[i] == cc[j] and crun[i] != crun[j] and R.iou(cb[i], cb[j]) >= thr + 0.01 for i, j in pairs)
    if design is DESIGN_DECISIONS:
        assert any(cc[i] == cc[j] and 0 < R.iou(cb[i], cb[j]) <= thr - 0.01 for i, j in pairs)
        assert any(cc[i] != cc[j] and R.iou(cb[i], cb[j]) > 0.99 for i, j in pairs)
        assert any(cc[i] == cc[j] and cs[i] == cs[j] and crun[i] != crun[j] and R.iou(cb[i], cb[j]) > thr for i, j in pairs)
    want = R.nms_topk(cb, cs, cc, thr, max_keep)
    assert len(want) == n_expected
    if max_keep == 5:
        assert len(R.nms_topk(cb, cs, cc, thr, 100)) > 5              # more survivors than max_keep
    # candidate index of the restatement -> slot of the padded layout (every designed row is valid)
    slot_of = [a * D + d for a, r in enumerate(runs) for d in range(len(r[3]))]
    boxes, scores, classes = _merge(cuda, runs, [OUT_HW], len(runs), D)
    keep, nkeep = HF.batched_nms_topk(boxes, scores, classes, thr, max_keep)
    n = int(nkeep[0])
    got = keep[0, :n].cpu().tolist()
    assert got == [slot_of[i] for i in want], (got, [slot_of[i] for i in want])
    kb, ks, kc = boxes[0, got].cpu().numpy(), scores[0, got].cpu().numpy(), classes[0, got].cpu().numpy()
    assert np.abs(kb - cb[want]).max() <= _tol(120) and (ks == cs[want].astype(np.float32)).all() and (kc == cc[want]).all()
    if design is DESIGN_DECISIONS:      # the tie went to run 0
        tie = [i for i in want if cs[i] == np.float32(0.6)]
        assert len(tie) == 1 and crun[tie[0]] == 0


# ------------------------------------------------------------------------------------------------ 3. the wrapper around a stub model
MEAN, STD = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]


def _stub_model(cuda, per_run):
    from slenderobjdet_amd.modeling.meta_arch.fcos import FCOSV2
    from slenderobjdet_amd.structures import PreparedInputs

    class Stub(FCOSV2):
        """The attributes GeneralizedRCNNWithTTA reads, nothing else; records what it is fed, returns the prescribed Instances."""

        def __init__(self):
            torch.nn.Module.__init__(self)
            self.register_buffer("pixel_mean", torch.zeros(3, 1, 1))
            self._mean, self._std = MEAN, STD
            self.backbone = torch.nn.Identity()
            self.backbone.size_divisibility = 32
            self.nms_thresh = 0.5
            self.calls, self.modes, self.served = [], [], 0

        def forward(self, batched_inputs):
            assert isinstance(batched_inputs, PreparedInputs)
            assert self.preprocess_image(batched_inputs) is batched_inputs.images
            self.calls.append(batched_inputs)
            self.modes.append(self.training)
            out = []
            for _ in batched_inputs:
                out.append({"instances": per_run[self.served]})
                self.served += 1
            return out

    return Stub().to(cuda)


def _instances(cuda, hw, boxes, scores, classes):
    from slenderobjdet_amd.structures import Boxes, Instances

    r = Instances(tuple(hw))
    r.pred_boxes = Boxes(torch.from_numpy(np.asarray(boxes, dtype=np.float32).reshape(-1, 4)).to(cuda))
    r.scores = torch.from_numpy(np.asarray(scores, dtype=np.float32).reshape(-1)).to(cuda)
    r.pred_classes = torch.from_numpy(np.asarray(classes, dtype=np.int64).reshape(-1)).to(cuda)
    return r


def _tta_cfg(cfg, min_sizes, flip, dets=100):
    cfg.TEST.AUG.MIN_SIZES, cfg.TEST.AUG.MAX_SIZE, cfg.TEST.AUG.FLIP = tuple(min_sizes), 4000, flip
    cfg.TEST.DETECTIONS_PER_IMAGE = dets
    return cfg


def _assert_final(inst, want, out_hw, tol):
    wb, ws, wc = want
    assert inst.image_size == tuple(out_hw) and len(inst) == len(ws), (len(inst), len(ws))
    assert inst.pred_classes.dtype == torch.int64 and (inst.pred_classes.cpu().numpy() == wc).all()
    assert (inst.scores.cpu().numpy() == ws.astype(np.float32)).all()
    if len(ws):
        assert np.abs(inst.pred_boxes.tensor.cpu().numpy() - wb).max() <= tol


def test_wrapper_around_stub_model(cuda):
    from slenderobjdet_amd.config import fresh_cfg
    from slenderobjdet_amd.data import DeviceInputPipeline
    from slenderobjdet_amd.modeling.test_time_augmentation import GeneralizedRCNNWithTTA, tta_plan

    cfg = _tta_cfg(fresh_cfg(), (40, 56), True)
    g = torch.Generator().manual_seed(11)
    image = torch.randint(0, 256, (3, 48, 64), dtype=torch.uint8, generator=g)
    plan = tta_plan(48, 64, (40, 56), 4000, True)
    assert plan == [(40, 53, False), (40, 53, True), (56, 75, False), (56, 75, True)] == R.plan(48, 64, (40, 56), 4000, True)
    out_hw = (96, 128)                                   # the requested output size differs from the image's
    augs = [((h, w), f) for h, w, f in plan]
    design = [(a % 4, box, s, c) for a, (_, box, s, c) in enumerate(DESIGN_DECISIONS)]
    design = [(a, (b[0] * 128 / 96, b[1] * 96 / 64, b[2] * 128 / 96, b[3] * 96 / 64), s, c) for a, b, s, c in design]
    runs = _runs_from_design(design, augs, out_hw)
    rr = [(r[2], r[3], r[4], r[5], r[6]) for r in runs]
    cb, cs, cc, _ = R.merge_candidates(rr, out_hw, 1e-8)
    assert R.same_class_iou_margin(cb, cc, 0.5) >= 0.01
    per_run = [_instances(cuda, r[5], r[2], r[3], r[4]) for r in runs]
    stub = _stub_model(cuda, per_run)
    stub.train()                                         # the wrapper runs the model in eval mode and restores the mode
    tta = GeneralizedRCNNWithTTA(cfg, stub, batch_size=3)
    out = tta([{"image": image, "height": out_hw[0], "width": out_hw[1]}])
    assert len(out) == 1 and stub.training and stub.modes == [False, False]
    assert [len(c) for c in stub.calls] == [3, 1]
    pipe = DeviceInputPipeline(pixel_mean=MEAN, pixel_std=STD, size_divisibility=32)
    hwc = image.to(cuda).permute(1, 2, 0).contiguous()
    for call, group in zip(stub.calls, (plan[:3], plan[3:])):
        ref, sizes, _, _ = pipe([hwc] * len(group), choices=group)
        assert call.images.image_sizes == sizes == [(h, w) for h, w, _ in group]
        assert [(d["height"], d["width"]) for d in call] == sizes
        assert call.images.tensor.dtype == torch.bfloat16 and torch.equal(call.images.tensor, ref)
    first = stub.calls[0].images.tensor
    assert torch.equal(first[1, :40, :53], first[0, :40, :53].flip(1))                 # the flipped run mirrors its twin
    assert torch.equal(stub.calls[1].images.tensor[0, :56, :75], pipe([hwc], choices=[(56, 75, False)])[0][0, :56, :75].flip(1))
    _assert_final(out[0]["instances"], R.tta(rr, out_hw, 1e-8, 0.5, 100), out_hw, _tol(128))
    assert len(out[0]["instances"]) == 5

    # all runs empty; height / width default to the image's own shape
    empty = [_instances(cuda, (h, w), np.zeros((0, 4)), np.zeros(0), np.zeros(0)) for h, w, _ in plan]
    res = GeneralizedRCNNWithTTA(cfg, _stub_model(cuda, empty))([{"image": image}])[0]["instances"]
    assert len(res) == 0 and res.image_size == (48, 64) and tuple(res.pred_boxes.tensor.shape) == (0, 4)


# ------------------------------------------------------------------------------------------------ 4. real models
def _build_real(arch):
    from bench import make_cfg
    from slenderobjdet_amd.modeling import build_model

    shrink_anchors = False
    if arch == "fcos":
        cfg = make_cfg(18)
        cfg.MODEL.FCOS.INFERENCE_TH = 0.005            # random init: class scores sit at the 0.01 prior
    elif arch == "retinanet":
        cfg = make_cfg(18, "retinanet")
        cfg.MODEL.RETINANET.SCORE_THRESH_TEST = 0.005
        shrink_anchors = True
    else:
        from test_gpu_rcnn import _cfg as rcnn_cfg       # the axis-aligned R-CNN as tests/test_gpu_rcnn.py builds it

        cfg = rcnn_cfg(rotated=False)
        cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0      # random init: every class probability is about 1 / 81
    cfg.TEST.DETECTIONS_PER_IMAGE = 8                    # few candidates per run: few pairs for the margin assertion below
    torch.manual_seed(3)
    model = build_model(cfg)
    if shrink_anchors:
        # A random-init RetinaNet returns its anchors (deltas about 0), 32 .. 813 px on a 64 x 96 image.  It suppresses the UNCLIPPED boxes
        # and clips afterwards (retina_rotated.py:296-377): clipped to the image, survivors of different anchors nearly coincide, and any
        # later NMS - the merging one included - drops all but one (measured on an MI355X: 8 returned, 7 kept at the identity plan).
        # With dw = dh = -2 the boxes are 0.135 x the anchors and mostly inside the image, as a trained model's are.
        with torch.no_grad():
            model.head.bbox_pred.bias[:36].view(9, 4)[:, 2:] = -2.0
        model.arena.bump()
    model.eval()
    return cfg, model


def _capture(model):
    """Forward hook: the PreparedInputs of every call and the (boxes, scores, classes, (h, w)) the model returned per run."""
    fed, got = [], []

    def hook(_m, args, output):
        fed.append(args[0])
        for o in output:
            r = o["instances"]
            got.append((r.pred_boxes.tensor.cpu().numpy().copy(), r.scores.cpu().numpy().copy(), r.pred_classes.cpu().numpy().copy(), r.image_size))

    return fed, got, model.register_forward_hook(hook)


# float32 IoU of class-shifted boxes: batched NMS adds class * (max coordinate + 1) <= 80 * 97 < 8192 to every coordinate, where a float32
# rounds by up to 2^-12 px, so a box side or an intersection side is off by up to 2^-11 px.  With sides >= 1 px (asserted) an area moves
# by at most 2 * 2^-11 relative and the IoU, a ratio of three such areas that is at most 1, by less than 8 * 2^-11 = 2^-8.  Decisions are
# compared only after asserting twice that margin in float64.
IOU_MARGIN = 2.0 ** -7


@pytest.mark.parametrize("arch", ["fcos", "rcnn", "retinanet"])
def test_real_models(cuda, arch):
    from slenderobjdet_amd.data import DeviceInputPipeline
    from slenderobjdet_amd.modeling.test_time_augmentation import GeneralizedRCNNWithTTA

    cfg, model = _build_real(arch)
    g = torch.Generator().manual_seed(17)
    image = torch.randint(0, 256, (3, 64, 96), dtype=torch.uint8, generator=g).to(cuda)
    with torch.no_grad():
        plain = model([{"image": image}])[0]["instances"]
    assert len(plain) >= 5                               # the lowered thresholds make the random-init model fire

    # 4a. identity plan.  The wrapper's result is compared with what the model returned for the one prepared batch it was run on (the SAME
    # forward pass: GroupNorm sums use float atomics, a second pass differs in the last bits).  The un-mapping is exact here (scale 1.0, boxes
    # already inside the image) and NMS at the model's own threshold keeps all of the model's survivors - asserted on the restatement
    # first - so the two results are identical, bit for bit.
    tta = GeneralizedRCNNWithTTA(_tta_cfg(cfg, (64,), False, 8), model)
    fed, got, handle = _capture(model)
    try:
        inst = tta([{"image": image}])[0]["instances"]
    finally:
        handle.remove()
    assert len(fed) == 1 and len(got) == 1 and fed[0].images.image_sizes == [(64, 96)]
    pipe = DeviceInputPipeline(pixel_mean=model._mean, pixel_std=model._std, size_divisibility=model.backbone.size_divisibility)
    assert torch.equal(fed[0].images.tensor, pipe([image.permute(1, 2, 0).contiguous()], choices=[(64, 96, False)])[0])
    b, s, c, size = got[0]
    assert len(s) >= 5 and size == (64, 96) and inst.image_size == (64, 96)
    margin = R.same_class_iou_margin(b.astype(np.float64), c, tta.nms_thresh)
    side = float(np.minimum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]).min())
    keep = R.nms_topk(b.astype(np.float64), s, c, tta.nms_thresh, 8)
    print(f"\n{arch}: identity run {len(s)} detections (plain {len(plain)}), smallest side {side:.3f} px, smallest same-class |IoU - threshold| "
          f"{margin:.4f}, the restated NMS keeps {len(keep)}, the wrapper {len(inst)}")
    assert side >= 1.0 and margin >= IOU_MARGIN
    assert keep == list(range(len(s)))                   # its own survivors do not suppress each other
    assert len(inst) == len(keep) and (inst.pred_classes.cpu().numpy() == c[keep]).all()
    assert torch.equal(inst.pred_boxes.tensor.cpu(), torch.from_numpy(b[keep])) and torch.equal(inst.scores.cpu(), torch.from_numpy(s[keep]))

    # 4b. two sizes with flip: the result is the restatement applied to the per-run outputs
    tta = GeneralizedRCNNWithTTA(_tta_cfg(cfg, (48, 64), True, 8), model)
    fed, got, handle = _capture(model)
    try:
        inst = tta([{"image": image}])[0]["instances"]
    finally:
        handle.remove()
    plan = R.plan(64, 96, (48, 64), 4000, True)
    assert [len(f) for f in fed] == [3, 1] and [r[3] for r in got] == [(h, w) for h, w, _ in plan]
    runs = [(r[0], r[1], r[2], (h, w), f) for r, (h, w, f) in zip(got, plan)]
    assert sum(len(r[1]) for r in runs) >= 5
    cb, cs, cc, _ = R.merge_candidates(runs, (64, 96), 1e-8)
    margin = R.same_class_iou_margin(cb, cc, tta.nms_thresh)
    side = float(np.minimum(cb[:, 2] - cb[:, 0], cb[:, 3] - cb[:, 1]).min())
    print(f"{arch}: {len(cs)} candidates, smallest side {side:.3f} px, NMS threshold {tta.nms_thresh}, smallest same-class |IoU - threshold| {margin:.4f}")
    assert side >= 1.0 and margin >= IOU_MARGIN
    want = R.tta(runs, (64, 96), 1e-8, tta.nms_thresh, 8)
    _assert_final(inst, want, (64, 96), _tol(96))
    bx, sc = inst.pred_boxes.tensor.cpu(), inst.scores.cpu()
    assert 1 <= len(inst) <= 8 and torch.isfinite(bx).all() and torch.isfinite(sc).all()
    assert (bx[:, 0::2] >= 0).all() and (bx[:, 0::2] <= 96).all() and (bx[:, 1::2] >= 0).all() and (bx[:, 1::2] <= 64).all()
    assert (sc[:-1] >= sc[1:]).all()


# ------------------------------------------------------------------------------------------------ 5. the prepared-batch hook
def test_plain_lists_take_the_path_they_always_took(cuda):
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.structures import ImageList, PreparedInputs

    cfg, model = _build_real("fcos")
    g = torch.Generator().manual_seed(2)
    data = [{"image": torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g).to(cuda)} for h, w in ((64, 96), (50, 70))]
    with torch.no_grad():
        images = model.preprocess_image(data)
    # decoded uint8 images in eval mode: the raw batch the fused stem consumes, as before
    assert type(images) is ImageList and isinstance(images.tensor, HF.RawImageBatch) and images.image_sizes == [(64, 96), (50, 70)]
    assert images.tensor.padded_hw == (64, 96) and all(torch.equal(a, d["image"]) for a, d in zip(images.tensor.imgs, data))
    want = torch.empty((2, 64, 96, 8), dtype=torch.bfloat16, device=cuda)
    HF.preprocess_batch([d["image"] for d in data], want, model._mean, model._std)
    assert torch.equal(images.tensor.materialize(), want)
    # float images: the NHWC(8) tensor itself
    with torch.no_grad():
        fl = model.preprocess_image([{"image": d["image"].float()} for d in data])
    want_f = torch.empty_like(want)
    HF.preprocess_batch([d["image"].float() for d in data], want_f, model._mean, model._std)
    assert type(fl) is ImageList and torch.is_tensor(fl.tensor) and fl.image_sizes == images.image_sizes and torch.equal(fl.tensor, want_f)
    # a prepared batch comes back as it is; one of the wrong dtype is refused
    prepared = PreparedInputs([{}, {}], ImageList(want, [(64, 96), (50, 70)]))
    assert model.preprocess_image(prepared) is prepared.images
    with pytest.raises(ValueError, match="NHWC"):
        model.preprocess_image(PreparedInputs([{}, {}], ImageList(want.float(), [(64, 96), (50, 70)])))
