"""The rotated GIoU loss without a GPU: the float64 restatement the GPU tests compare with (tests/rotated_giou_loss_restated.py) is
itself checked against central differences and closed forms; the config key builds; the new config loads; the C ABI declares the
symbols; the wrappers refuse CPU tensors."""
import os

import pytest
import torch

import rotated_giou_loss_restated as GL
import rotated_iou_loss_restated as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs", "rotated", "retinanet_rgiou_R_50_FPN_1x.yaml")
MAX_EXCLUDED = 0.04          # a condition: at most this share of the pairs may sit within 1e-2 px of a kink


def _central_differences(pred, gt, h=1e-5):
    fd = torch.zeros_like(pred)
    for e in range(5):
        d = torch.zeros(5, dtype=torch.float64)
        d[e] = h
        fd[:, e] = (GL.loss(pred + d, gt) - GL.loss(pred - d, gt)) / (2 * h)
    return fd


@pytest.mark.parametrize("seed", [0, 7])
def test_restated_gradient_equals_central_differences(seed):
    """Autograd through the float64 clipping and the shoelace sum over the hull's vertices against central differences (h = 1e-5) of
    the same loss on generate(512, seed) and generate_far(512, seed), rounded to float32 like the GPU tests' inputs: every row outside
    the exclusion mask within 1e-5 of its norm (measured 1.4e-8 / 1.4e-8 near, 8.6e-9 / 8.6e-9 far); at most 4 % excluded (measured
    1.95 % / 2.54 % near, 0.98 % / 0.39 % far).  In the far set at least 300 disjoint rows are compared (428 / 433 of 432 / 434), and
    none of them has a zero gradient: the hull term acts where 1 - IoU is flat."""
    for name, (pred, gt) in (("near", RL.generate(512, seed)), ("far", GL.generate_far(512, seed))):
        pred, gt = pred.float().double(), gt.float().double()
        _, g = GL.loss_and_grad(pred, gt)
        out = GL.excluded(pred, gt)
        disjoint = RL.iou(pred, gt) == 0
        share = float(out.double().mean())
        fd = _central_differences(pred, gt)
        err = ((g - fd).norm(dim=1) / g.norm(dim=1))[~out]
        print(f"\n{name} seed {seed}: {int(disjoint.sum())} disjoint ({int((disjoint & ~out).sum())} compared), {int(out.sum())} excluded "
              f"({100 * share:.2f} %), worst row {float(err.max()):.3g} of its norm over {int((~out).sum())} pairs")
        assert share <= MAX_EXCLUDED
        assert float(err.max()) <= 1e-5
        assert (g[disjoint & ~out].norm(dim=1) > 0).all()
        if name == "far":
            assert int((disjoint & ~out).sum()) >= 300
            _, gi = RL.loss_and_grad(pred, gt)
            assert (gi[disjoint] == 0).all()              # what 1 - IoU alone gives these rows


def _giou_xyxy(a, b):
    """fvcore's giou_loss of two XYXY boxes with eps = 0."""
    xk1, yk1, xk2, yk2 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    inter = (xk2 - xk1) * (yk2 - yk1) if xk2 > xk1 and yk2 > yk1 else 0.0
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    ac = (max(a[2], b[2]) - min(a[0], b[0])) * (max(a[3], b[3]) - min(a[1], b[1]))
    return 1.0 - (inter / union - (ac - union) / ac)


def test_restated_special_cases():
    pred, gt, forward_only, names = GL.special_cases()
    assert names[-3:] == ["shared_edge_line", "shared_edge_line_axis", "touching_hull_only"] and forward_only.tolist()[-3:] == [True, True, False]
    assert forward_only[names.index("identical")] and forward_only[names.index("swapped_90")]
    l, g = GL.loss_and_grad(pred, gt)
    by = dict(zip(names, l.tolist()))
    c = dict(zip(names, GL.hull_area(pred, gt).tolist()))
    assert abs(by["identical"]) < 1e-12 and abs(by["swapped_90"]) < 1e-12
    assert abs(c["pred_inside_gt"] - 480.0) < 1e-12 * 480 and abs(c["gt_inside_pred"] - 480.0) < 1e-12 * 480
    assert abs(by["shared_edge_line"] - GL.SHARED_EDGE_LINE_LOSS) < 1e-12 and abs(by["shared_edge_line_axis"] - GL.SHARED_EDGE_LINE_LOSS) < 1e-12
    assert abs(c["shared_edge_line"] - 488.0) < 1e-9 and abs(c["shared_edge_line_axis"] - 488.0) < 1e-9
    assert float((GL.hull_term_given_iou(pred, gt, RL.iou(pred, gt)) - GL.hull_term(pred, gt)).abs().max()) < 1e-12
    assert RL.iou(pred, gt)[names.index("touching_hull_only")] == 0 and 1.0 < by["touching_hull_only"] < 2.0
    # a prediction strictly inside its gt: hull = gt = union, so the hull term and its gradient vanish
    i = names.index("pred_inside_gt")
    ht, hg = GL.hull_term_and_grad(pred, gt)
    assert abs(float(ht[i])) < 1e-12 and float(hg[i].abs().max()) < 1e-12
    _, gi = RL.loss_and_grad(pred, gt)
    assert float((g[i] - gi[i]).abs().max()) < 1e-12
    # everything compared on the GPU is away from the kinks, and autograd is right there
    assert (GL.hull_margin(pred, gt)[~forward_only] >= 0.05).all() and (RL.margin(pred, gt)[~forward_only] >= 0.05).all()
    assert not GL.excluded(pred, gt)[~forward_only].any()
    fd = _central_differences(pred, gt)
    assert float((g - fd)[~forward_only].abs().max()) <= 1e-7
    assert g[names.index("disjoint")].norm() > 0 and g[names.index("touching_hull_only")].norm() > 0


def test_axis_aligned_pairs_equal_giou_of_their_xyxy_forms():
    """Angle 0: the hull of two axis-aligned boxes is NOT their enclosing box in general, but it is when one box's x range and the
    other's y range contain the other's (a cross), when one contains the other and when they share an extent; for such pairs the loss
    is fvcore's GIoU of the XYXY forms, to 1e-12."""
    rows = [([50.0, 40.0, 30.0, 8.0, 0.0], [50.0, 40.0, 30.0, 8.0, 0.0]),            # identical
            ([50.0, 40.0, 30.0, 8.0, 0.0], [52.0, 41.0, 10.0, 4.0, 0.0]),            # contained
            ([50.0, 40.0, 30.0, 8.0, 0.0], [58.0, 40.0, 30.0, 8.0, 0.0]),            # shifted along x, same y extent
            ([50.0, 40.0, 30.0, 8.0, 0.0], [95.0, 40.0, 30.0, 8.0, 0.0]),            # the same, disjoint
            ([50.0, 40.0, 8.0, 30.0, 0.0], [50.0, 61.0, 8.0, 10.0, 0.0])]            # stacked along y, same x extent, disjoint
    pred = torch.tensor([r[0] for r in rows], dtype=torch.float64)
    gt = torch.tensor([r[1] for r in rows], dtype=torch.float64)
    xyxy = lambda b: [b[0] - b[2] / 2, b[1] - b[3] / 2, b[0] + b[2] / 2, b[1] + b[3] / 2]
    want = torch.tensor([_giou_xyxy(xyxy(r[0]), xyxy(r[1])) for r in rows], dtype=torch.float64)
    got = GL.loss(pred, gt)
    assert float((got - want).abs().max()) < 1e-12, (got, want)
    # and in general the hull is no larger than the enclosing box: loss <= GIoU
    a, b = [50.0, 40.0, 30.0, 8.0, 0.0], [60.0, 50.0, 10.0, 20.0, 0.0]
    l = float(GL.loss(torch.tensor([a], dtype=torch.float64), torch.tensor([b], dtype=torch.float64)))
    assert l < _giou_xyxy(xyxy(a), xyxy(b))


def test_loss_range():
    sp, sg, _, _ = GL.special_cases()
    pn, gn = RL.generate(512, 3)
    pf, gf = GL.generate_far(512, 3)
    l = GL.loss(torch.cat([sp, pn, pf]), torch.cat([sg, gn, gf]))
    assert float(l.min()) >= -1e-12 and float(l.max()) < 2.0
    assert (GL.hull_term(torch.cat([sp, pn, pf]), torch.cat([sg, gn, gf])) >= -1e-12).all()


def _cfg(arch_yaml=YAML):
    from slenderobjdet_amd.config import fresh_cfg

    cfg = fresh_cfg()
    cfg.merge_from_file(arch_yaml)
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def test_new_config_loads():
    cfg = _cfg()
    assert cfg.MODEL.META_ARCHITECTURE == "RotatedRetinaNet" and cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE == "rotated_giou"
    base = _cfg(os.path.join(ROOT, "configs", "rotated", "retinanet_R_50_FPN_1x.yaml"))
    assert base.MODEL.RETINANET.BBOX_REG_LOSS_TYPE == "smooth_l1"
    base.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "rotated_giou"
    assert base.dump() == cfg.dump()              # the one key is the only difference


def test_build_model_accepts_rotated_giou_only_for_the_rotated_class():
    from slenderobjdet_amd.modeling import build_model

    torch.manual_seed(0)
    m = build_model(_cfg())
    assert type(m).__name__ == "RotatedRetinaNet" and m.box_reg_loss_type == "rotated_giou"
    assert m.box_reg_loss_types == ("smooth_l1", "rotated_iou", "rotated_giou")
    cfg = _cfg(os.path.join(ROOT, "configs", "retina", "retinanet_R_50_FPN_1x.yaml"))
    assert cfg.MODEL.META_ARCHITECTURE == "RetinaNet"
    cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "rotated_giou"
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    assert "MODEL.RETINANET.BBOX_REG_LOSS_TYPE" in str(e.value) and "RetinaNet" in str(e.value)
    cfg = _cfg()
    cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "giou"
    with pytest.raises(ValueError) as e:
        build_model(cfg)
    assert all(v in str(e.value) for v in ("'smooth_l1'", "'rotated_iou'", "'rotated_giou'"))


def test_cabi_declares_the_loss_kernels():
    from slenderobjdet_amd import _C
    from test_cabi_surface import _declared

    decl = _declared()
    for name, sibling in (("sod_rotated_giou_loss", "sod_rotated_iou_loss"), ("sod_retina_rgiou_loss_fwd", "sod_retina_riou_loss_fwd"),
                          ("sod_retina_rgiou_loss_bwd", "sod_retina_riou_loss_bwd"), ("sod_retina_rgiou_loss_bwd_f32", "sod_retina_riou_loss_bwd_f32")):
        assert decl[name] == decl[sibling] == len(_C._SIGS[name]), name
        assert _C._SIGS[name] == _C._SIGS[sibling], name
    assert "rotated_iou_loss.hip" in open(os.path.join(ROOT, "slenderobjdet_amd", "csrc", "Makefile")).read()       # the pair operator's file


def test_layers_exports_the_loss_without_loading_it_with_the_package():
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, %r); import slenderobjdet_amd.layers.functional; "
            "assert 'slenderobjdet_amd.layers.losses' not in sys.modules; "
            "from slenderobjdet_amd.layers import rotated_giou_loss; from slenderobjdet_amd.layers.losses import rotated_giou_loss as f; "
            "assert rotated_giou_loss is f; from slenderobjdet_amd.layers import rotated_iou_loss as r; assert r is not f; "
            "import slenderobjdet_amd.layers as L; assert not hasattr(L, 'no_such_name')") % ROOT
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_wrappers_refuse_cpu_tensors():
    """No silent fall-back: the op layer rejects CPU tensors, and so does the autograd function built on it."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.layers import rotated_giou_loss

    a, b = torch.rand(3, 5) + 1, torch.rand(3, 5) + 1
    with pytest.raises(_C.SlenderHipError):
        HF.rotated_giou_loss_fwd(a, b)
    with pytest.raises(_C.SlenderHipError):
        HF.rotated_giou_loss_bwd(a, b)
    with pytest.raises(_C.SlenderHipError):
        rotated_giou_loss(a.requires_grad_(True), b)
    with pytest.raises(ValueError):
        rotated_giou_loss(a, b, reduction="median")
    with pytest.raises(ValueError):
        rotated_giou_loss(a[:, :4], b[:, :4])
    n = torch.zeros(1)
    with pytest.raises(_C.SlenderHipError):
        HF.retina_rgiou_loss_fwd(torch.zeros(1, 4, 8), 8, torch.zeros(1, 4, dtype=torch.int32), torch.zeros(4, 5), torch.zeros(1, 4, 5), 1, 4, 1, 8,
                                 (1.0,) * 5, 4.0, n, 0.9)
