"""RotatedRetinaNet without a GPU: the config builds, the refusals name their key, the C ABI declares the kernels, and the CPU
restatement (tests/rotated_retinanet_restated.py) gives the hand-made cases of the model's semantics."""
import math
import os

import pytest
import torch

import rotated_retinanet_restated as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs", "rotated", "retinanet_R_50_FPN_1x.yaml")
W5 = (1.0, 1.0, 1.0, 1.0, 1.0)


def _cfg():
    from slenderobjdet_amd.config import fresh_cfg

    cfg = fresh_cfg()
    cfg.merge_from_file(YAML)
    cfg.MODEL.DEVICE = "cpu"
    return cfg


@pytest.fixture(scope="module")
def cpu_model():
    from slenderobjdet_amd.modeling import build_model

    torch.manual_seed(0)
    return build_model(_cfg())


def test_rotated_retinanet_builds_from_repo_config_cpu(cpu_model):
    from slenderobjdet_amd.modeling import META_ARCH_REGISTRY, RotatedRetinaNet
    from slenderobjdet_amd.modeling.meta_arch import RetinaNet

    m = cpu_model
    assert "RotatedRetinaNet" in META_ARCH_REGISTRY
    assert type(m).__name__ == "RotatedRetinaNet" and isinstance(m, RotatedRetinaNet)
    assert not isinstance(m, RetinaNet)           # test-time augmentation takes a RetinaNet's boxes for XYXY
    A = 18
    assert m.head.num_anchors == A and m.head.box_dim == 5 and m.head.kc == A * 80 == 1440
    assert m.head.bbox_pred.ckpt_rows == A * 5 and m.head.box_pitch == 96 and m.head.cls_score.ckpt_rows == 1440
    w = m.head.bbox_pred.weight.detach()
    assert w.shape[0] == 96 and (w[A * 5:] == 0).all() and w[: A * 5].abs().sum() > 0
    assert m.bbox_reg_weights == W5 and m.anchor_angles == [[-90, -60, -30, 0, 30, 60]]
    anc = m.anchors_for([(2, 3), (1, 2), (1, 1), (1, 1), (1, 1)])
    assert anc.shape == (11 * A, 5)
    ref = RS.anchors([(2, 3), (1, 2), (1, 1), (1, 1), (1, 1)], m.strides, m.anchor_sizes, m.anchor_ratios, m.anchor_angles)
    assert torch.equal(anc, ref)


def test_axis_aligned_head_keeps_its_layout():
    """box_dim defaults to 4: 9 anchors -> 36 real rows in a 40-row bbox_pred, as before."""
    from slenderobjdet_amd.config import fresh_cfg
    from slenderobjdet_amd.modeling.meta_arch import RetinaNetHead

    cfg = fresh_cfg()
    h = RetinaNetHead(cfg, 256, 9)
    assert h.box_dim == 4 and h.box_pitch == 40 and h.bbox_pred.ckpt_rows == 36 and (h.bbox_pred.weight.detach()[36:] == 0).all()


@pytest.mark.parametrize("edit, needle", [
    (lambda c: setattr(c.MODEL.ANCHOR_GENERATOR, "NAME", "DefaultAnchorGenerator"), "MODEL.ANCHOR_GENERATOR.NAME"),
    (lambda c: setattr(c.MODEL.RETINANET, "BBOX_REG_WEIGHTS", (1.0, 1.0, 1.0, 1.0)), "MODEL.RETINANET.BBOX_REG_WEIGHTS"),
    (lambda c: setattr(c.MODEL.RETINANET, "BBOX_REG_LOSS_TYPE", "giou"), "MODEL.RETINANET.BBOX_REG_LOSS_TYPE"),
    (lambda c: setattr(c.MODEL.RETINANET, "NUM_CLASSES", 3), "MODEL.RETINANET.NUM_CLASSES"),
])
def test_refusals_name_their_key(edit, needle):
    from slenderobjdet_amd.modeling import build_model

    cfg = _cfg()
    edit(cfg)
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    assert needle in str(e.value) and "RotatedRetinaNet" in str(e.value)


def test_tta_refuses_five_column_boxes(cpu_model):
    from slenderobjdet_amd.modeling import GeneralizedRCNNWithTTA

    with pytest.raises(ValueError) as e:
        GeneralizedRCNNWithTTA(_cfg(), cpu_model)
    assert "RotatedRetinaNet is not supported" in str(e.value)


def test_cabi_declares_the_rotated_retina_kernels():
    from slenderobjdet_amd import _C
    from test_cabi_surface import _declared

    decl = _declared()
    for name, n in (("sod_retina_label_rotated", 19), ("sod_retina_box5_loss_fwd", 14), ("sod_retina_box5_loss_bwd", 13),
                    ("sod_retina_box5_loss_bwd_f32", 13), ("sod_retina_decode_rotated", 16)):
        assert decl[name] == n == len(_C._SIGS[name]), name
    text = open(os.path.join(ROOT, "include", "slender_hip.h")).read()
    assert "SOD_RETINA_LABEL_MAX_GT" in text and "rotated_retina.hip" in text
    assert "rotated_retina.hip" in open(os.path.join(ROOT, "slenderobjdet_amd", "csrc", "Makefile")).read()


def test_wrappers_refuse_cpu_tensors():
    """No silent fall-back: the op layer rejects CPU tensors."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    with pytest.raises(_C.SlenderHipError):
        HF.retina_label_rotated(torch.zeros(4, 5), torch.zeros(1, 1, 5), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                                [0.4, 0.5], [0, -1, 1], True, 8, W5)
    with pytest.raises(_C.SlenderHipError):
        HF.retina_decode_rotated(torch.zeros(1, 4, 8), torch.zeros(4, 5), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2), 1, [4], 2, W5, 4.0)


# ------------------------------------------------------------------------------------------------ the restatement's hand-made cases
K = 8


def _label(anc, gts, cls):
    return RS.label_anchors(anc, gts, cls, [0.4, 0.5], [0, -1, 1], K, W5, dtype=torch.float64)


def test_restated_anchor_equal_to_a_gt():
    anc = torch.tensor([[50.0, 40.0, 30.0, 10.0, 30.0], [200.0, 200.0, 20.0, 20.0, 0.0]])
    lab, d, _ = _label(anc, [anc[:1].clone()], [torch.tensor([5])])
    assert lab[0].tolist() == [5, K]
    assert torch.equal(d[0, 0], torch.zeros(5, dtype=torch.float64))


def test_restated_angle_difference_wraps():
    """anchor at 170 degrees, gt at -170 degrees: the short way round is +20 degrees, not -340."""
    anc = torch.tensor([[64.0, 64.0, 40.0, 40.0, 170.0]])
    gt = torch.tensor([[64.0, 64.0, 40.0, 40.0, -170.0]])
    lab, d, q = _label(anc, [gt], [torch.tensor([2])])
    assert lab[0].tolist() == [2] and float(q[0][0, 0]) > 0.5
    assert d[0, 0, :4].abs().max() == 0
    assert abs(float(d[0, 0, 4]) - 20.0 * math.pi / 180.0) < 1e-12


def test_restated_low_quality_match_promotes_the_best_anchor():
    anc = torch.tensor([[20.0, 20.0, 32.0, 32.0, 0.0], [36.0, 20.0, 32.0, 32.0, 0.0], [300.0, 300.0, 32.0, 32.0, 0.0]])
    gt = torch.tensor([[60.0, 20.0, 32.0, 32.0, 0.0]])            # overlaps anchor 1 by 8 x 32: IoU 256 / 1792 = 1 / 7
    lab, d, q = _label(anc, [gt], [torch.tensor([3])])
    assert abs(float(q[0][0, 1]) - 1.0 / 7.0) < 1e-6 and float(q[0].max()) < 0.4
    assert lab[0].tolist() == [K, 3, K]
    assert abs(float(d[0, 1, 0]) - 24.0 / 32.0) < 1e-12


def test_restated_empty_image_and_losses():
    anc = torch.tensor([[20.0, 20.0, 32.0, 32.0, 0.0], [36.0, 20.0, 32.0, 32.0, 45.0]])
    lab, d, _ = _label(anc, [torch.zeros(0, 5)], [torch.zeros(0, dtype=torch.int64)])
    assert lab[0].tolist() == [K, K] and d.abs().max() == 0 and d.shape == (1, 2, 5)
    logits = torch.zeros(1, 2, K, dtype=torch.float64)
    out, norm = RS.losses(logits, torch.ones(1, 2, 5, dtype=torch.float64), lab, d, K, 0.25, 2.0, 0.1, 100.0)
    assert float(out["loss_box_reg"]) == 0.0 and abs(norm - 90.1) < 1e-12             # 0.9 * 100 + 0.1 * max(0, 1)
    assert abs(float(out["loss_cls"]) - 2 * K * 0.75 * 0.25 * math.log(2.0) / 90.1) < 1e-12


def test_restated_decode_clamps_and_wraps():
    anc = torch.tensor([[10.0, 20.0, 8.0, 4.0, 170.0]], dtype=torch.float64)
    d = torch.tensor([[0.5, -0.5, 100.0, 0.0, 30.0 * math.pi / 180.0]], dtype=torch.float64)
    b = RS.apply_deltas(d, anc, W5)[0]
    assert abs(float(b[0]) - 14.0) < 1e-12 and abs(float(b[1]) - 18.0) < 1e-12
    assert abs(float(b[2]) - 8.0 * 1000.0 / 16) < 1e-9 and abs(float(b[3]) - 4.0) < 1e-12
    assert abs(float(b[4]) - (-160.0)) < 1e-9
