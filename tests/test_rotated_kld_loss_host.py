"""The Gaussian KL-divergence box loss ("rotated_kld") without a GPU: the closed form the kernel evaluates (csrc/gauss_box_loss.h) against
the float64 restatement built from the covariance matrices (tests/rotated_kld_loss_restated.py), the properties of the loss on that
restatement, the config value on every model family, the refusals, the new configs and the C ABI."""
import math
import os

import pytest
import torch

import rotated_kld_loss_restated as KL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT = os.path.join(ROOT, "configs", "rotated")
F64 = torch.float64


def closed_form(p, t):
    """The closed form of csrc/gauss_box_loss.h and its hand-written gradient in float64 -> (L (P), dL / dp (P, 5), angle per degree)."""
    r = math.pi / 180.0
    wp, hp, wt, ht = p[:, 2], p[:, 3], t[:, 2], t[:, 3]
    tt, dl = t[:, 4] * r, (p[:, 4] - t[:, 4]) * r
    ct, st, cd, sd = torch.cos(tt), torch.sin(tt), torch.cos(dl), torch.sin(dl)
    dx, dy = p[:, 0] - t[:, 0], p[:, 1] - t[:, 1]
    u, v = dx * ct - dy * st, dx * st + dy * ct
    D = (2 * (u / wt) ** 2 + 2 * (v / ht) ** 2 + 0.5 * ((wp * cd / wt) ** 2 + (hp * sd / wt) ** 2 + (wp * sd / ht) ** 2 + (hp * cd / ht) ** 2)
         + torch.log(wt * ht / (wp * hp)) - 1)
    L = 1 - 1 / (1 + torch.log1p(D.clamp_min(0)))
    dLdD = 1 / ((1 + torch.log1p(D)) ** 2 * (1 + D))
    g = torch.stack([4 * u * ct / wt ** 2 + 4 * v * st / ht ** 2, -4 * u * st / wt ** 2 + 4 * v * ct / ht ** 2,
                     wp * (cd ** 2 / wt ** 2 + sd ** 2 / ht ** 2) - 1 / wp, hp * (sd ** 2 / wt ** 2 + cd ** 2 / ht ** 2) - 1 / hp,
                     0.5 * torch.sin(2 * dl) * (hp ** 2 - wp ** 2) * (1 / wt ** 2 - 1 / ht ** 2) * r], 1)
    return L, g * dLdD[:, None]


# ------------------------------------------------------------------------------------------------ 1. closed form
def test_closed_form_equals_the_matrix_definition():
    """1 000 near and 1 000 far seeded pairs, rounded to float32 and lifted: the closed form's value within 1e-10 of the restatement's,
    its hand-written gradient rows within 1e-10 of the row norm of float64 autograd through inv / logdet (measured 4.9e-15 and 1.4e-13).
    The special cases too, the sliver apart (see the next test); rows whose exact gradient is zero count by their absolute error."""
    pred, gt = KL.pairs(1000, 1000)
    assert pred.shape == (2000, 5)
    ref_l, ref_g = KL.loss_and_grad(pred, gt)
    l, g = closed_form(pred, gt)
    err_l = float((l - ref_l).abs().max())
    row = float(((g - ref_g).norm(dim=1) / ref_g.norm(dim=1)).max())
    print(f"\nclosed form against the matrices: value {err_l:.3g}, worst gradient row {row:.3g} of its norm")
    assert err_l <= 1e-10 and row <= 1e-10
    sp, sg, names = KL.special_cases()
    ref_l, ref_g = KL.loss_and_grad(sp, sg)
    l, g = closed_form(sp, sg)
    keep = torch.tensor([n != "sliver" for n in names])          # the sliver's covariance has condition 3e17: float64 inv loses digits there
    err_l, row, _ = KL.row_errors(l[keep], g[keep], ref_l[keep], ref_g[keep])          # rows with an exactly zero gradient: absolute
    assert err_l <= 1e-10 and row <= 1e-10


def test_sliver_value_from_the_matrices_at_fifty_digits():
    """The sliver pair (gt 8000 x 1.5e-5 px): its covariance has condition number 2.8e17, so float64 cannot even hold the assembled matrix -
    the restatement's inv / logdet give 0.9718 there.  The same matrix definition evaluated with 50 digits (mpmath) is the arbiter of
    this one pair: 0.97016578, the constant KL.SLIVER_LOSS the GPU test compares with; the float64 closed form agrees to 1e-9."""
    import mpmath as mp

    mp.mp.dps = 50
    sp, sg, names = KL.special_cases()
    i = names.index("sliver")
    p, t = [mp.mpf(float(x)) for x in sp[i]], [mp.mpf(float(x)) for x in sg[i]]

    def gaussian(b):
        a = b[4] * mp.pi / 180
        rot = mp.matrix([[mp.cos(a), mp.sin(a)], [-mp.sin(a), mp.cos(a)]])
        return mp.matrix([b[0], b[1]]), rot * mp.matrix([[b[2] ** 2 / 4, 0], [0, b[3] ** 2 / 4]]) * rot.T

    (mp_, sp_), (mt, st) = gaussian(p), gaussian(t)
    inv = st ** -1
    d = mp_ - mt
    prod = inv * sp_
    kld = (d.T * inv * d)[0] / 2 + (prod[0, 0] + prod[1, 1]) / 2 + mp.log(mp.det(st) / mp.det(sp_)) / 2 - 1
    want = 1 - 1 / (1 + mp.log(1 + kld))
    l, _ = closed_form(sp[i:i + 1], sg[i:i + 1])
    ref = float(KL.loss(sp[i:i + 1], sg[i:i + 1]))
    print(f"\nsliver: 50 digits {float(want):.10f}, float64 closed form {float(l):.10f}, float64 matrices {ref:.6f}, KL divergence {float(kld):.4g}")
    assert abs(float(want) - KL.SLIVER_LOSS) <= 1e-8 and abs(float(l) - float(want)) <= 1e-9
    assert 0.0 < ref < 1.0


# ------------------------------------------------------------------------------------------------ 2. properties, on the restatement
def test_identical_boxes_have_zero_loss_and_gradient():
    b = KL.lift(torch.tensor([[33.0, 44.0, 28.0, 7.0, -17.0], [10.0, 20.0, 5.0, 5.0, 30.0], [64.0, 64.0, 100.0, 2.0, 33.0]], dtype=F64))
    l, g = KL.loss_and_grad(b, b)
    assert float(l.abs().max()) <= 1e-12 and float(g.abs().max()) <= 1e-10


def test_invariant_to_how_a_box_is_written():
    """(w, h, t) against (h, w, t + 90), t against t +- 180: one Gaussian, so one value - for the prediction and for the gt."""
    pred, gt = KL.pairs(256, 256, 3, 3)
    base = KL.loss(pred, gt)
    swap = lambda b: torch.stack([b[:, 0], b[:, 1], b[:, 3], b[:, 2], b[:, 4] + 90.0], 1)
    turn = lambda b, d: torch.cat([b[:, :4], b[:, 4:] + d], 1)
    for other in (KL.loss(swap(pred), gt), KL.loss(pred, swap(gt)), KL.loss(turn(pred, 180.0), gt), KL.loss(turn(pred, -180.0), gt),
                  KL.loss(pred, turn(gt, 180.0)), KL.loss(pred, turn(gt, -180.0))):
        assert float((other - base).abs().max()) <= 1e-12


def test_loss_range():
    sp, sg, _ = KL.special_cases()
    pred, gt = KL.pairs(512, 512, 3, 3)
    l = KL.loss(torch.cat([sp, pred]), torch.cat([sg, gt]))
    assert float(l.min()) >= -1e-12 and float(l.max()) < 1.0          # float64 rounding at the identical boxes: -2e-16


def test_disjoint_pair_is_pulled_to_its_gt():
    """Centres ten box lengths apart: the centre gradient points from the gt to the prediction, so descent moves the prediction to the gt;
    for a displacement along one of the gt's axes it is parallel to it."""
    gt = KL.lift(torch.tensor([[100.0, 100.0, 40.0, 8.0, 25.0]], dtype=F64))
    t = 25.0 * math.pi / 180.0
    for dirn in ((1.0, 0.0), (0.0, 1.0), (0.6, -0.8), (math.cos(t), -math.sin(t)), (math.sin(t), math.cos(t))):
        pred = gt.clone()
        pred[0, 0] += 400.0 * dirn[0]
        pred[0, 1] += 400.0 * dirn[1]
        l, g = KL.loss_and_grad(pred, gt)
        dot = float(g[0, 0] * dirn[0] + g[0, 1] * dirn[1])
        assert 0.0 < float(l) < 1.0 and dot > 0.0 and float(g[0, :2].norm()) > 0.0
        stepped = pred.clone()
        stepped[0, :2] -= 1.0 * g[0, :2] / g[0, :2].norm()
        assert float((stepped[0, :2] - gt[0, :2]).norm()) < float((pred[0, :2] - gt[0, :2]).norm())
    assert abs(dot / float(g[0, :2].norm()) - 1.0) <= 1e-9          # the last two directions are the gt's own axes


def test_angle_gradient_grows_with_the_aspect_ratio():
    """Equal centres and sizes, 3 degrees of angle error, a 100 px long side at ratios 1, 2, 5, 10, 50: dL / d angle is 0 for the square
    and strictly increasing after it - 0, 0.0020, 0.0192, 0.0622, 0.0834 per degree."""
    vals = []
    for ratio in KL.RATIOS:
        _, g = KL.loss_and_grad(*KL.slender(ratio))
        vals.append(float(g[0, 4]))
    print("\ndL / d angle per degree at ratios", KL.RATIOS, [round(v, 4) for v in vals])
    assert abs(vals[0]) <= 1e-12
    assert all(b > a for a, b in zip(vals, vals[1:]))
    assert [round(v, 4) for v in vals] == [0.0, 0.0020, 0.0192, 0.0622, 0.0834]


# ------------------------------------------------------------------------------------------------ 3. config
def _yaml_cfg(path):
    from slenderobjdet_amd.config import fresh_cfg

    cfg = fresh_cfg()
    cfg.merge_from_file(path)
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def test_new_configs_load():
    cfg = _yaml_cfg(os.path.join(ROT, "retinanet_rkld_R_50_FPN_1x.yaml"))
    assert cfg.MODEL.META_ARCHITECTURE == "RotatedRetinaNet" and cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE == "rotated_kld"
    base = _yaml_cfg(os.path.join(ROT, "retinanet_R_50_FPN_1x.yaml"))
    assert base.MODEL.RETINANET.BBOX_REG_LOSS_TYPE == "smooth_l1"
    base.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "rotated_kld"
    assert base.dump() == cfg.dump()                   # the one key is the only difference
    cfg = _yaml_cfg(os.path.join(ROT, "faster_rkld_R_101.yaml"))
    assert cfg.MODEL.META_ARCHITECTURE == "GeneralizedRCNN" and cfg.MODEL.ROI_HEADS.NAME == "RROIHeads" and cfg.MODEL.PROPOSAL_GENERATOR.NAME == "RRPN"
    assert cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE == cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE == "rotated_kld"
    base = _yaml_cfg(os.path.join(ROT, "faster_R_101.yaml"))
    assert base.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE == base.MODEL.RPN.BBOX_REG_LOSS_TYPE == "smooth_l1"
    base.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = "rotated_kld"
    assert base.dump() != cfg.dump()
    base.MODEL.RPN.BBOX_REG_LOSS_TYPE = "rotated_kld"
    assert base.dump() == cfg.dump()                   # the two keys are the only difference


def _same_parameters(a, b):
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(pa) == list(pb)                        # the loss type adds no parameter and moves none
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def test_rotated_retinanet_builds_with_the_value():
    from slenderobjdet_amd.modeling import build_model
    from test_gpu_rotated_iou_loss import _cfg

    models = {}
    for value in ("smooth_l1", "rotated_kld"):
        cfg = _cfg(value)
        cfg.MODEL.DEVICE = "cpu"
        torch.manual_seed(0)
        models[value] = build_model(cfg)
    m = models["rotated_kld"]
    assert type(m).__name__ == "RotatedRetinaNet" and m.box_reg_loss_type == "rotated_kld"
    assert "rotated_kld" in m.box_reg_loss_types + m.gauss_box_reg_loss_types
    _same_parameters(models["smooth_l1"], m)
    cfg = _cfg("rotated_kl")
    cfg.MODEL.DEVICE = "cpu"
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    assert "MODEL.RETINANET.BBOX_REG_LOSS_TYPE" in str(e.value) and "'rotated_kld'" in str(e.value)


def test_rotated_rcnn_builds_with_the_value_on_either_stage():
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.modeling.box_regression import BOX_REG_LOSS_TYPES
    from test_gpu_rcnn import _cfg

    assert BOX_REG_LOSS_TYPES[5][-1] == "rotated_kld" and "rotated_kld" not in BOX_REG_LOSS_TYPES[4]

    def build(roi, rpn):
        cfg = _cfg(True)
        cfg.MODEL.DEVICE = "cpu"
        cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE, cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE = roi, rpn
        torch.manual_seed(0)
        return build_model(cfg)

    base = build("smooth_l1", "smooth_l1")
    for roi, rpn in (("rotated_kld", "smooth_l1"), ("smooth_l1", "rotated_kld"), ("rotated_kld", "rotated_kld")):
        m = build(roi, rpn)
        assert type(m.roi_heads).__name__ == "RROIHeads" and type(m.proposal_generator).__name__ == "RRPN"
        assert m.roi_heads.box_predictor.box_reg_loss_type == roi and m.proposal_generator.box_reg_loss_type == rpn
        _same_parameters(base, m)


def test_axis_aligned_models_refuse_the_value_and_name_their_key():
    from slenderobjdet_amd.modeling import build_model
    from test_gpu_anchor_head import _cfg as anchor_head_cfg
    from test_gpu_rcnn import _cfg as rcnn_cfg

    cfg = _yaml_cfg(os.path.join(ROOT, "configs", "retina", "retinanet_R_50_FPN_1x.yaml"))
    assert cfg.MODEL.META_ARCHITECTURE == "RetinaNet"
    cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "rotated_kld"
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    assert "MODEL.RETINANET.BBOX_REG_LOSS_TYPE" in str(e.value) and "RetinaNet" in str(e.value) and "'rotated_kld'" in str(e.value)
    cfg = anchor_head_cfg("none", "rotated_kld")
    cfg.MODEL.DEVICE = "cpu"
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    assert "MODEL.META_ARCH.BBOX_REG_LOSS_TYPE" in str(e.value) and "AnchorHead" in str(e.value) and "'rotated_kld'" in str(e.value)
    for key, name in (("ROI_BOX_HEAD", "StandardROIHeads"), ("RPN", "RPN")):
        cfg = rcnn_cfg(False)
        cfg.MODEL.DEVICE = "cpu"
        cfg.MODEL[key].BBOX_REG_LOSS_TYPE = "rotated_kld"
        with pytest.raises(ValueError) as e:
            build_model(cfg)
        assert f"MODEL.{key}.BBOX_REG_LOSS_TYPE" in str(e.value) and name in str(e.value) and "'rotated_kld'" in str(e.value)


# ------------------------------------------------------------------------------------------------ 4. C ABI and wrappers
def test_cabi_declares_the_entries_and_the_kind():
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF
    from test_cabi_surface import _declared

    decl = _declared()
    for name, sibling in (("sod_rotated_kld_loss", "sod_rotated_giou_loss"), ("sod_retina_rkld_loss_fwd", "sod_retina_rgiou_loss_fwd"),
                          ("sod_retina_rkld_loss_bwd", "sod_retina_rgiou_loss_bwd"), ("sod_retina_rkld_loss_bwd_f32", "sod_retina_rgiou_loss_bwd_f32")):
        assert decl[name] == decl[sibling] == len(_C._SIGS[name]), name
        assert _C._SIGS[name] == _C._SIGS[sibling], name
    header = open(os.path.join(ROOT, "include", "slender_hip.h")).read()
    assert "#define SOD_BOX_LOSS_ROTATED_KLD 3" in header
    assert HF.ROWS_GAUSS_LOSS_KINDS == {"rotated_kld": (3, 5)}
    csrc = os.path.join(ROOT, "slenderobjdet_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "rotated_kld_loss.hip" in mk and "gauss_box_loss.h" in mk
    # one definition: the pair operator and the two fused skeletons include the header, the policy lives in box_loss_policy.h alone, and
    # the chain from the box gradient to the delta gradient is written once
    for f in ("rotated_kld_loss.hip", "retina_box_loss.hip", "rows_box_loss.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "gauss_box_loss.h"' in src and "struct RkldLoss" not in src and "rkld_pair(" not in src.replace("rkld_pair<", "")
    policy = open(os.path.join(csrc, "box_loss_policy.h")).read()
    assert "struct RkldLoss" in policy and policy.count("180.f / (SOD_PI") == 1 and policy.count("rot_delta_grad(gb, s, box, k, a.w.w, g)") == 2
    assert "rot_pts" not in open(os.path.join(csrc, "rotated_kld_loss.hip")).read()          # no clipping points in LDS


def test_wrappers_refuse_cpu_tensors():
    """No silent fall-back: the op layer rejects CPU tensors, and so does the autograd function built on it."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.layers import rotated_kld_loss
    from slenderobjdet_amd.layers.losses import rotated_kld_loss as f

    assert rotated_kld_loss is f
    a, b = torch.rand(3, 5) + 1, torch.rand(3, 5) + 1
    with pytest.raises(_C.SlenderHipError):
        HF.rotated_kld_loss_fwd(a, b)
    with pytest.raises(_C.SlenderHipError):
        HF.rotated_kld_loss_bwd(a, b)
    with pytest.raises(_C.SlenderHipError):
        rotated_kld_loss(a.requires_grad_(True), b)
    with pytest.raises(ValueError):
        rotated_kld_loss(a, b, reduction="median")
    with pytest.raises(ValueError):
        rotated_kld_loss(a[:, :4], b[:, :4])
    n = torch.zeros(1)
    with pytest.raises(_C.SlenderHipError):
        HF.retina_rkld_loss_fwd(torch.zeros(1, 4, 8), 8, torch.zeros(1, 4, dtype=torch.int32), torch.zeros(4, 5), torch.zeros(1, 4, 5), 1, 4, 1, 8,
                                (1.0,) * 5, 4.0, n, 0.9)
    with pytest.raises(_C.SlenderHipError):
        HF.rows_box_loss_fwd("rotated_kld", "frcnn", torch.zeros(4, 16), torch.zeros(4, dtype=torch.int32), 3, torch.zeros(4, 5), torch.zeros(4, 5),
                             (10.0, 10.0, 5.0, 5.0, 1.0), 4.0)
