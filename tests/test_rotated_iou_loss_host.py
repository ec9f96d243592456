"""The rotated IoU loss without a GPU: the float64 restatement the GPU tests compare with (tests/rotated_iou_loss_restated.py) is
itself checked against central differences; the config key builds; the new config loads; the wrappers refuse CPU tensors."""
import os

import pytest
import torch

import rotated_iou_loss_restated as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs", "rotated", "retinanet_riou_R_50_FPN_1x.yaml")
MARGIN = 1e-2                # px: pairs closer than this to a change of the intersection's structure are left out
MAX_EXCLUDED = 0.03


def _central_differences(pred, gt, h=1e-5):
    fd = torch.zeros_like(pred)
    for e in range(5):
        d = torch.zeros(5, dtype=torch.float64)
        d[e] = h
        fd[:, e] = ((1 - RL.iou(pred + d, gt)) - (1 - RL.iou(pred - d, gt))) / (2 * h)
    return fd


@pytest.mark.parametrize("seed", [0, 7])
def test_restated_gradient_equals_central_differences(seed):
    """Autograd through the float64 clipping against central differences (h = 1e-5) of the same IoU on generate(512, seed): every row
    within 1e-5 of its norm outside the margin (measured 4.9e-9 on 4 096 pairs); at most 3 % of the pairs are inside the margin
    (measured 1.6 % - 1.7 %; another 1.5 % - 1.9 % are disjoint); disjoint pairs are NOT excluded: their gradient is exactly zero."""
    pred, gt = RL.generate(512, seed)
    loss, g = RL.loss_and_grad(pred, gt)
    m = RL.margin(pred, gt)
    disjoint = loss == 1.0
    near = (m < MARGIN) & ~disjoint
    share = float(near.double().mean())
    fd = _central_differences(pred, gt)
    assert (g[disjoint] == 0).all() and (fd[disjoint] == 0).all()
    keep = ~near & ~disjoint
    err = ((g - fd).norm(dim=1) / g.norm(dim=1))[keep]
    print(f"\nseed {seed}: {int(disjoint.sum())} disjoint, {int(near.sum())} inside the margin ({100 * share:.2f} %), "
          f"worst row {float(err.max()):.3g} of its norm over {int(keep.sum())} pairs")
    assert share <= MAX_EXCLUDED
    assert int(keep.sum()) >= 450 and float(err.max()) <= 1e-5


def test_restated_special_cases():
    pred, gt, forward_only, names = RL.special_cases()
    v = RL.iou(pred, gt)
    by = dict(zip(names, v.tolist()))
    assert by["disjoint"] == 0.0
    assert abs(by["identical"] - 1.0) < 1e-12 and abs(by["swapped_90"] - 1.0) < 1e-12
    assert abs(by["pred_inside_gt"] - 30.0 / 480.0) < 1e-12 and abs(by["gt_inside_pred"] - 30.0 / 480.0) < 1e-12
    assert all(0.0 <= x <= 1.0 + 1e-12 for x in by.values())
    m = RL.margin(pred, gt)
    assert (m[~forward_only] >= 0.05).all(), dict(zip(names, m.tolist()))
    _, g = RL.loss_and_grad(pred, gt)
    fd = _central_differences(pred, gt)
    check = ~forward_only
    assert float((g - fd)[check].abs().max()) <= 1e-7
    assert (g[names.index("disjoint")] == 0).all()
    # a prediction strictly inside its gt: moving it changes nothing, growing it raises the IoU
    i = names.index("pred_inside_gt")
    assert g[i, 0] == 0 and g[i, 1] == 0 and g[i, 2] < 0 and g[i, 3] < 0


def _cfg(arch_yaml=YAML):
    from slenderobjdet_amd.config import fresh_cfg

    cfg = fresh_cfg()
    cfg.merge_from_file(arch_yaml)
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def test_new_config_loads():
    cfg = _cfg()
    assert cfg.MODEL.META_ARCHITECTURE == "RotatedRetinaNet" and cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE == "rotated_iou"
    base = _cfg(os.path.join(ROOT, "configs", "rotated", "retinanet_R_50_FPN_1x.yaml"))
    assert base.MODEL.RETINANET.BBOX_REG_LOSS_TYPE == "smooth_l1"
    base.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "rotated_iou"
    assert base.dump() == cfg.dump()              # the one key is the only difference


def test_build_model_accepts_rotated_iou_only_for_the_rotated_class():
    from slenderobjdet_amd.modeling import build_model

    torch.manual_seed(0)
    m = build_model(_cfg())
    assert type(m).__name__ == "RotatedRetinaNet" and m.box_reg_loss_type == "rotated_iou"
    cfg = _cfg(os.path.join(ROOT, "configs", "retina", "retinanet_R_50_FPN_1x.yaml"))
    assert cfg.MODEL.META_ARCHITECTURE == "RetinaNet"
    cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "rotated_iou"
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    assert "MODEL.RETINANET.BBOX_REG_LOSS_TYPE" in str(e.value) and "RetinaNet" in str(e.value)


def test_cabi_declares_the_loss_kernels():
    from slenderobjdet_amd import _C
    from test_cabi_surface import _declared

    decl = _declared()
    for name, n in (("sod_rotated_iou_loss", 9), ("sod_retina_riou_loss_fwd", 16), ("sod_retina_riou_loss_bwd", 15),
                    ("sod_retina_riou_loss_bwd_f32", 15), ("sod_retina_label_rotated_boxes", 19)):
        assert decl[name] == n == len(_C._SIGS[name]), name
    assert _C._SIGS["sod_retina_riou_loss_fwd"] == _C._SIGS["sod_retina_giou_loss_fwd"]
    assert _C._SIGS["sod_retina_label_rotated_boxes"] == _C._SIGS["sod_retina_label_rotated"]
    assert "rotated_iou_loss.hip" in open(os.path.join(ROOT, "slenderobjdet_amd", "csrc", "Makefile")).read()


def test_layers_exports_the_loss_without_loading_it_with_the_package():
    """``layers.rotated_iou_loss`` resolves on first use: importing a sub-module of ``layers`` (every model does) loads what it loaded
    before the export existed."""
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, %r); import slenderobjdet_amd.layers.functional; "
            "assert 'slenderobjdet_amd.layers.losses' not in sys.modules; "
            "from slenderobjdet_amd.layers import rotated_iou_loss; from slenderobjdet_amd.layers.losses import rotated_iou_loss as f; "
            "assert rotated_iou_loss is f; import slenderobjdet_amd.layers as L; "
            "assert not hasattr(L, 'no_such_name')") % ROOT
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_wrappers_refuse_cpu_tensors():
    """No silent fall-back: the op layer rejects CPU tensors, and so does the autograd function built on it."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.layers import rotated_iou_loss

    a, b = torch.rand(3, 5) + 1, torch.rand(3, 5) + 1
    with pytest.raises(_C.SlenderHipError):
        HF.rotated_iou_loss_fwd(a, b)
    with pytest.raises(_C.SlenderHipError):
        HF.rotated_iou_loss_bwd(a, b)
    with pytest.raises(_C.SlenderHipError):
        rotated_iou_loss(a.requires_grad_(True), b)
    with pytest.raises(ValueError):
        rotated_iou_loss(a, b, reduction="median")
    with pytest.raises(ValueError):
        rotated_iou_loss(a[:, :4], b[:, :4])
