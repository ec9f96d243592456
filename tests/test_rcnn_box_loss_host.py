"""MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE / BBOX_REG_LOSS_WEIGHT and MODEL.RPN.BBOX_REG_LOSS_TYPE without a GPU: the value sets by box type
and the refusals that name their key; the default config builds what it built; the new configs load; the C ABI, the ctypes table and
the Makefile carry the row kernels; the wrappers refuse CPU tensors; the float64 restatement the GPU tests compare with
(tests/rcnn_box_loss_restated.py) reproduces hand-computed GIoU cases and its input recipe stays under the exclusion cap."""
import os

import pytest
import torch

import rcnn_box_loss_restated as RR
import rotated_giou_loss_restated as GL
import rotated_iou_loss_restated as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT = os.path.join(ROOT, "configs", "rotated")
MAX_EXCLUDED = 0.04          # a condition: at most this share of the rows may sit within 1e-2 px of a kink


def _cfg(yaml=None, rotated=True):
    """The rotated R-CNN config file, or the small two-stage model of the GPU tests (R18; axis-aligned when not ``rotated``)."""
    from slenderobjdet_amd.config import fresh_cfg

    if yaml is not None:
        cfg = fresh_cfg()
        cfg.merge_from_file(os.path.join(ROT, yaml))
    else:
        from test_gpu_rcnn import _cfg as small

        cfg = small(rotated)
    cfg.MODEL.DEVICE = "cpu"
    return cfg


ALLOWED = {False: ("smooth_l1", "giou"), True: ("smooth_l1", "rotated_iou", "rotated_giou")}
HEADS = {False: ("StandardROIHeads", "RPN"), True: ("RROIHeads", "RRPN")}


@pytest.mark.parametrize("rotated", [False, True])
def test_value_sets_by_box_type(rotated):
    """Every allowed value builds, on either stage alone; the objects carry it."""
    from slenderobjdet_amd.modeling import build_model

    roi_name, rpn_name = HEADS[rotated]
    for value in ALLOWED[rotated]:
        for stage in ("roi", "rpn"):
            cfg = _cfg(rotated=rotated)
            if stage == "roi":
                cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = value
            else:
                cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE = value
            torch.manual_seed(0)
            m = build_model(cfg)
            assert type(m.roi_heads).__name__ == roi_name and type(m.proposal_generator).__name__ == rpn_name
            assert m.roi_heads.box_predictor.box_reg_loss_type == (value if stage == "roi" else "smooth_l1")
            assert m.proposal_generator.box_reg_loss_type == (value if stage == "rpn" else "smooth_l1")


@pytest.mark.parametrize("rotated, value", [(False, "rotated_iou"), (False, "rotated_giou"), (False, "diou"), (False, "ciou"),
                                            (True, "giou"), (True, "diou"), (True, "ciou"), (True, "smooth_l2")])
def test_refusals_name_their_key(rotated, value):
    """A value outside the box type's set raises ValueError when the model is built; the message names the key, the class and the
    allowed values."""
    from slenderobjdet_amd.modeling import build_model

    assert value not in ALLOWED[rotated]
    roi_name, rpn_name = HEADS[rotated]
    cfg = _cfg(rotated=rotated)
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = value
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    msg = str(e.value)
    assert "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE" in msg and roi_name in msg and repr(value) in msg
    assert all(repr(v) in msg for v in ALLOWED[rotated])
    cfg = _cfg(rotated=rotated)
    cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE = value
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    msg = str(e.value)
    assert "MODEL.RPN.BBOX_REG_LOSS_TYPE" in msg and rpn_name in msg and repr(value) in msg
    assert all(repr(v) in msg for v in ALLOWED[rotated])


def test_default_config_builds_the_same_objects():
    """The defaults are smooth_l1 with weight 1.0: same parameters (names, shapes, values for a seed) as a config that spells them out,
    and the loss weights of the RPN are what they were."""
    from slenderobjdet_amd.modeling import build_model

    for rotated in (False, True):
        cfg = _cfg(rotated=rotated)
        assert cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE == cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE == "smooth_l1"
        assert cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT == 1.0
        torch.manual_seed(0)
        a = build_model(cfg)
        pred, rpn = a.roi_heads.box_predictor, a.proposal_generator
        assert pred.box_reg_loss_type == rpn.box_reg_loss_type == "smooth_l1" and pred.box_reg_loss_weight == 1.0
        assert rpn.loss_weight == {"loss_rpn_cls": 1.0, "loss_rpn_loc": 1.0}
        cfg2 = _cfg(rotated=rotated)
        cfg2.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = ALLOWED[rotated][-1]
        cfg2.MODEL.RPN.BBOX_REG_LOSS_TYPE = ALLOWED[rotated][-1]
        cfg2.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT = 2.0
        torch.manual_seed(0)
        b = build_model(cfg2)
        assert b.roi_heads.box_predictor.box_reg_loss_weight == 2.0
        pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
        assert list(pa) == list(pb)                    # the loss type adds no parameter and moves none
        for k in pa:
            assert torch.equal(pa[k], pb[k]), k


def test_cls_agnostic_stays_unbuilt():
    from slenderobjdet_amd.modeling import build_model

    cfg = _cfg(rotated=True)
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    with pytest.raises(NotImplementedError):
        build_model(cfg)


@pytest.mark.parametrize("yaml, value", [("faster_riou_R_101.yaml", "rotated_iou"), ("faster_rgiou_R_101.yaml", "rotated_giou")])
def test_new_configs_load(yaml, value):
    cfg = _cfg(yaml)
    assert cfg.MODEL.META_ARCHITECTURE == "GeneralizedRCNN" and cfg.MODEL.ROI_HEADS.NAME == "RROIHeads"
    assert cfg.MODEL.PROPOSAL_GENERATOR.NAME == "RRPN"
    assert cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE == cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE == value
    base = _cfg("faster_R_101.yaml")
    assert base.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE == base.MODEL.RPN.BBOX_REG_LOSS_TYPE == "smooth_l1"
    base.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = value
    assert base.dump() != cfg.dump()
    base.MODEL.RPN.BBOX_REG_LOSS_TYPE = value
    assert base.dump() == cfg.dump()                   # the two keys are the only difference


def test_cabi_declares_the_row_kernels():
    from slenderobjdet_amd import _C
    from test_cabi_surface import _declared

    decl = _declared()
    assert decl["sod_rows_box_loss_fwd"] == len(_C._SIGS["sod_rows_box_loss_fwd"]) == 14
    assert decl["sod_rows_box_loss_bwd"] == len(_C._SIGS["sod_rows_box_loss_bwd"]) == 15
    assert _C._SIGS["sod_rows_box_loss_bwd"][:11] == _C._SIGS["sod_rows_box_loss_fwd"][:11]
    header = open(os.path.join(ROOT, "include", "slender_hip.h")).read()
    for name in ("SOD_ROWS_FRCNN 0", "SOD_ROWS_RPN 1", "SOD_BOX_LOSS_GIOU 0", "SOD_BOX_LOSS_ROTATED_IOU 1", "SOD_BOX_LOSS_ROTATED_GIOU 2"):
        assert "#define " + name in header
    mk = open(os.path.join(ROOT, "slenderobjdet_amd", "csrc", "Makefile")).read()
    assert "rows_box_loss.hip" in mk and "box_loss_policy.h" in mk
    # one definition of the policies: the two kernel files include the header and neither defines a policy itself
    csrc = os.path.join(ROOT, "slenderobjdet_amd", "csrc")
    for f in ("rows_box_loss.hip", "retina_box_loss.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "box_loss_policy.h"' in src and "struct GiouLoss" not in src and "struct RotIouLoss" not in src
    from slenderobjdet_amd.layers import functional as HF

    assert HF.ROWS_BOX_LOSS_KINDS == {"giou": (0, 4), "rotated_iou": (1, 5), "rotated_giou": (2, 5)}


def test_wrappers_refuse_cpu_tensors():
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    pred, src, gt = torch.zeros(4, 16), torch.zeros(4, 5), torch.zeros(4, 5)
    lab32, lab8 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int8)
    one = torch.ones(1)
    with pytest.raises(_C.SlenderHipError):
        HF.rows_box_loss_fwd("rotated_iou", "frcnn", pred, lab32, 3, src, gt, RR.W_ROI5, RR.SCALE_CLAMP)
    with pytest.raises(_C.SlenderHipError):
        HF.rows_box_loss_bwd("rotated_giou", "rpn", pred[:, :5].contiguous(), lab8, 1, src, gt, RR.W_ROI5, RR.SCALE_CLAMP, one, 1.0)
    with pytest.raises(_C.SlenderHipError):
        HF.rows_box_loss_fwd("giou", "frcnn", pred, lab32, 4, src[:, :4].contiguous(), gt[:, :4].contiguous(), (10.0, 10.0, 5.0, 5.0), RR.SCALE_CLAMP)
    with pytest.raises(_C.SlenderHipError):
        HF.rows_box_loss_fwd("diou", "frcnn", pred, lab32, 3, src, gt, RR.W_ROI5, RR.SCALE_CLAMP)


def test_restated_giou_hand_computed_cases():
    """identical boxes: 0; two unit squares two apart (gap 1): IoU 0, enclosing box 3 x 1, union 2 -> 1 - 0 + (3 - 2) / 3 = 4 / 3;
    a 1 x 1 box inside a 2 x 2 box: IoU 1 / 4, the enclosing box is the union -> 3 / 4.  (eps 1e-7 moves these by < 1e-6.)"""
    b1 = torch.tensor([[0.0, 0.0, 2.0, 3.0], [0.0, 0.0, 1.0, 1.0], [0.5, 0.5, 1.5, 1.5]], dtype=torch.float64)
    b2 = torch.tensor([[0.0, 0.0, 2.0, 3.0], [2.0, 0.0, 3.0, 1.0], [0.0, 0.0, 2.0, 2.0]], dtype=torch.float64)
    got = RR.giou_xyxy(b1, b2)
    want = torch.tensor([0.0, 4.0 / 3.0, 0.75], dtype=torch.float64)
    assert float((got - want).abs().max()) < 1e-6, got
    # the decode is the inverse of get_deltas, and the row selection reads the gt class's columns
    g = torch.Generator().manual_seed(2)
    c, wh = torch.rand(7, 2, generator=g, dtype=torch.float64) * 100, 5 + torch.rand(7, 2, generator=g, dtype=torch.float64) * 40
    src = torch.cat([c - wh / 2, c + wh / 2], 1)
    tgt = src + torch.rand(7, 4, generator=g, dtype=torch.float64) * 2
    w = (10.0, 10.0, 5.0, 5.0)
    d = RR.get_deltas_xyxy(src, tgt, w)
    assert float((RR.decode_xyxy(d, src, w) - tgt).abs().max()) < 1e-9
    K = 3
    pred = torch.full((7, 16), 1e3, dtype=torch.float64)
    labels = torch.tensor([0, 1, 2, 3, -1, 2, 0], dtype=torch.int32)
    for i, l in enumerate(labels.tolist()):
        if 0 <= l < K:
            pred[i, l * 4:l * 4 + 4] = d[i]
    total, grad, fg, boxes = RR.rows_loss("giou", "frcnn", pred, labels, K, src, src, w)
    assert fg.tolist() == [True, True, True, False, False, True, True]
    assert abs(total - float(RR.giou_xyxy(tgt[fg], src[fg]).sum())) < 1e-9
    assert (grad[~fg] == 0).all() and (grad[:, 12:] == 0).all() and (grad[0, 4:] == 0).all() and grad[0, :4].abs().sum() > 0
    total8, _, fg8, _ = RR.rows_loss("giou", "rpn", d, torch.tensor([1, 0, -1, 1, 1, 0, 1], dtype=torch.int8), 1, src, src, w)
    assert fg8.tolist() == [True, False, False, True, True, False, True]
    assert abs(total8 - float(RR.giou_xyxy(tgt[fg8], src[fg8]).sum())) < 1e-9


@pytest.mark.parametrize("near, far", [(192, 192), (96, 96)])
def test_rotated_row_recipe_stays_under_the_exclusion_cap(near, far):
    """The rotated rows of the GPU test: a foreground row decodes to its wanted box (float32 rounding of the deltas apart); at most 4 %
    of the foreground rows lie within 1e-2 px of a kink (measured 7 of 330, 2.1 %; with 96 + 96: 1 of 165), and a good third of them
    does not overlap its gt box (139 of 330): the rows on which "rotated_iou" has no gradient and "rotated_giou" has one."""
    pred, labels, src, gt = RR.rotated_rows(near, far)
    R = near + far
    assert pred.shape == (R, 16) and pred.dtype == torch.float32 and labels.dtype == torch.int32 and src.shape == gt.shape == (R, 5)
    assert (labels[6::7] == 3).all() and int((labels == 3).sum()) == R // 7 and set(labels.tolist()) == {0, 1, 2, 3}
    assert bool(torch.isfinite(pred).all()) and float(pred[:, 15].abs().min()) > 0
    _, _, fg, boxes = RR.rows_loss("rotated_giou", "frcnn", pred, labels, 3, src, gt, RR.W_ROI5)
    wn, _ = RL.generate(near, 11)
    wf, _ = GL.generate_far(far, 13)
    wanted = torch.cat([wn, wf]).float().double()[fg]
    dev = boxes - wanted
    dev[:, 4] = (dev[:, 4] + 180.0) % 360.0 - 180.0
    assert float(dev.abs().max()) < 1e-3
    out = GL.excluded(boxes, gt.double()[fg])
    apart = RL.iou(boxes, gt.double()[fg]) == 0
    share = float(out.double().mean())
    print(f"\n{near} + {far}: {int(fg.sum())} foreground rows, {int(out.sum())} within the margin of a kink ({100 * share:.2f} %), "
          f"{int(apart.sum())} without overlap")
    assert share <= MAX_EXCLUDED
    assert int(apart.sum()) >= int(fg.sum()) // 4 and int((~apart).sum()) >= int(fg.sum()) // 4
