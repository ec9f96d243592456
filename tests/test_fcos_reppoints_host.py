"""FCOSRepPoints, host side (CPU): the restatement (tests/fcos_reppoints_restated.py) against the fixtures the reference's own Python
produced (tests/golden/fcos_reppoints/, generator make_golden_fcos_reppoints.py), the registry entry, the head's parameter count and
the C-ABI table.  The kernels are checked against the same fixtures and the same restatement in tests/test_gpu_fcos_reppoints.py."""
import os

import numpy as np
import pytest
import torch

import fcos_reppoints_restated as RS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_reppoints")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLENDER_BOX = [23.1515, 45.727, 120.8485, 58.273]        # see test_slender_selection_differs_from_the_plain_one_on_a_slender_box


def load_gts(z):
    n = len([k for k in z.files if k.startswith("boxes")])
    return [torch.from_numpy(z[f"boxes{i}"]) for i in range(n)], [torch.from_numpy(z[f"classes{i}"]) for i in range(n)]


def level_hw(z):
    return [tuple(int(v) for v in r) for r in z["level_hw"]]


@pytest.mark.parametrize("name", ["targets_seed1.npz", "targets_seed2.npz"])
@pytest.mark.parametrize("radius", [1.5, 0.0])
def test_restated_targets_equal_the_reference(name, radius):
    z = np.load(os.path.join(GOLD, name))
    boxes, classes = load_gts(z)
    K = int(z["num_classes"])
    lab, reg, score, idx, sel = RS.slender_targets(level_hw(z), z["strides"].tolist(), boxes, classes, radius, K)
    assert torch.equal(lab, torch.from_numpy(z[f"gt_classes_r{radius}"]))
    assert torch.equal(reg, torch.from_numpy(z[f"reg_targets_r{radius}"]))
    assert torch.equal(sel, torch.from_numpy(z[f"topk_locations_r{radius}"]))
    ref = torch.from_numpy(z[f"scores_r{radius}"])       # torch.pow over other batch shapes: not bit-equal, 1e-6 as everywhere
    assert float((score - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) and bool(((score > 0) == (ref > 0)).all())
    fg = lab != K
    assert int(z[f"num_gt_over_topk_r{radius}"]) >= 2 and 0 < int(sel.sum()) < int(fg.sum())      # the cut is exercised
    assert bool((sel <= fg).all()) and bool(((idx >= 0) == fg).all())


def test_restated_ground_truth_equals_the_reference():
    z = np.load(os.path.join(GOLD, "ground_truth.npz"))
    boxes, classes = load_gts(z)
    K, hw, strides = int(z["num_classes"]), level_hw(z), z["strides"].tolist()
    lab, reg, _score, _idx, sel = RS.slender_targets(hw, strides, boxes, classes, float(z["radius"]), K)
    assert torch.equal(lab, torch.from_numpy(z["init_gt_classes"])) and torch.equal(reg, torch.from_numpy(z["init_reg_targets"]))
    assert torch.equal(sel, torch.from_numpy(z["topk_locations"]))
    sizes = [tuple(int(v) for v in r) for r in z["image_sizes"]]
    cls, ltrb, _m, mlab, _v = RS.refine_targets(hw, strides, torch.from_numpy(z["init_boxes"]), boxes, classes, sizes, K, z["thresholds"].tolist(),
                                                z["labels"].tolist())
    ref = torch.from_numpy(z["refine_gt_classes"])
    assert torch.equal(cls, ref) and torch.equal(ltrb, torch.from_numpy(z["refine_reg_targets"]))
    # image 0 fills the 128 x 160 batch (only the coarse levels' last locations, x = 192 / 224, lie outside); 1 is narrower, 2 lower
    outside = [int((ref[i] == -1).sum()) for i in range(3)]
    assert outside[0] == 3 and outside[1] > 40 and outside[2] > 40, outside
    assert bool(((mlab == 0) == (cls == K))[cls >= 0].all())      # only matcher label 0 is background: label -1 keeps the gt class (:356-357)


def test_restated_offsets2ltrb_equals_the_reference():
    z = np.load(os.path.join(GOLD, "offsets2ltrb.npz"))
    nl = len(level_hw(z))
    got = RS.offsets2ltrb([torch.from_numpy(z[f"points{l}"]) for l in range(nl)])
    for l in range(nl):
        assert torch.equal(got[l], torch.from_numpy(z[f"ltrb{l}"]))


@pytest.mark.parametrize("iou_type", ["giou", "iou"])
def test_restated_losses_equal_the_reference(iou_type):
    z = np.load(os.path.join(GOLD, f"losses_{iou_type}.npz"))
    boxes, classes = load_gts(z)
    K, hw, strides = int(z["num_classes"]), level_hw(z), z["strides"].tolist()
    nl = len(hw)
    lab, reg, _score, _idx, sel = RS.slender_targets(hw, strides, boxes, classes, float(z["radius"]), K)
    assert torch.equal(lab, torch.from_numpy(z["init_gt_classes"])) and torch.equal(sel, torch.from_numpy(z["topk_locations"]))
    preds = [[torch.from_numpy(z[f"{k}{l}"]).clone().requires_grad_(True) for l in range(nl)] for k in ("logits", "points_init", "points_refine", "ctrness")]
    init_ltrb, refine_ltrb = RS.ltrb_rows(RS.offsets2ltrb(preds[1])), RS.ltrb_rows(RS.offsets2ltrb(preds[2]))
    if iou_type == "iou":
        assert bool((init_ltrb[sel] > 0).all()) and bool((reg[sel] > 0).all())
    else:
        assert bool((init_ltrb[sel] < 0).any())
    sizes = [tuple(int(v) for v in r) for r in z["image_sizes"]]
    cls, rreg, _m, _l, _v = RS.refine_targets(hw, strides, RS.decode_boxes(init_ltrb.detach(), hw, strides), boxes, classes, sizes, K,
                                              z["thresholds"].tolist(), z["labels"].tolist())
    assert torch.equal(cls, torch.from_numpy(z["refine_gt_classes"])) and torch.equal(rreg, torch.from_numpy(z["refine_reg_targets"]))
    assert int(((cls >= 0) & (cls != K)).sum()) == int(z["num_refine_positives"]) > sum(len(b) for b in boxes)
    N = lab.shape[0]
    st = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(hw, strides)]).repeat(N)
    out = RS.rpd_losses(lab.reshape(-1), reg.reshape(-1, 4), sel.reshape(-1), cls.reshape(-1), rreg.reshape(-1, 4), RS.ltrb_rows(preds[0]).reshape(-1, K),
                        init_ltrb.reshape(-1, 4), refine_ltrb.reshape(-1, 4), RS.ltrb_rows(preds[3]).reshape(-1), st, K, float(z["alpha"]),
                        float(z["gamma"]), iou_type)
    assert sorted(out) == ["centerness_loss", "cls_loss", "reg_loss", "reg_loss_init"]
    for k, v in out.items():
        ref = float(z["loss::" + k])
        assert abs(float(v.detach()) - ref) <= 1e-5 * max(abs(ref), 1.0), (k, float(v.detach()), ref)
    flat = preds[0] + preds[1] + preds[2] + preds[3]
    grads = torch.autograd.grad(sum(out.values()), flat)
    names = [f"grad_{k}{l}" for k in ("logits", "points_init", "points_refine", "ctrness") for l in range(nl)]
    for n, g in zip(names, grads):
        ref = torch.from_numpy(z[n])
        assert float((g - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1.0), n


def test_slender_selection_differs_from_the_plain_one_on_a_slender_box():
    """Inside one box w / h is the same at every location, so the slender score c ** min(w/h, h/w) orders the positives as c (and its
    square root, FCOSTopK's score) does: the two selections can differ only where rounding decides.  This 97.7 x 12.5 box is such a
    case: locations 353 and 355 (stride 16) are mirror images about its centre, their c differ by rounding, the square root keeps
    them apart (355 wins) and the exponent 0.128 maps both to ONE float32 (the lower index 353 wins).  Both true powers lie within
    0.06 ulp of that float (checked in float64), so any powf good to 0.4 ulp gives the same tie."""
    from oracle import losses as ol

    hw, strides = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)], [8, 16, 32, 64, 128]
    box, cls = [torch.tensor([SLENDER_BOX])], [torch.tensor([3])]
    a = RS.slender_targets(hw, strides, box, cls, 0.0, 80)
    b = RS.slender_targets(hw, strides, box, cls, 0.0, 80, score=ol.centerness_targets)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert int(a[4].sum()) == int(b[4].sum()) == 5 and not torch.equal(a[4], b[4])
    only_a, only_b = (a[4] & ~b[4]).nonzero()[:, 1].tolist(), (b[4] & ~a[4]).nonzero()[:, 1].tolist()
    assert (only_a, only_b) == ([353], [355])
    assert float(a[2][0, 353]) == float(a[2][0, 355]) and float(b[2][0, 355]) > float(b[2][0, 353])
    reg = a[1][0, [353, 355]].double()
    q = (reg[:, 0] + reg[:, 2]).float() / (reg[:, 1] + reg[:, 3]).float()
    r = torch.minimum(q, 1 / q).double()
    c = ((reg[:, [0, 2]].min(1)[0].float() / reg[:, [0, 2]].max(1)[0].float()) * (reg[:, [1, 3]].min(1)[0].float() / reg[:, [1, 3]].max(1)[0].float())).double()
    true = torch.pow(c, r)
    ulp = float(np.spacing(np.float32(a[2][0, 353])))
    assert float((true - float(a[2][0, 353])).abs().max()) <= 0.06 * ulp


def test_build_model_resolves_fcos_reppoints():
    from slenderobjdet_amd.config import fresh_cfg
    from slenderobjdet_amd.modeling import META_ARCH_REGISTRY, build_model
    from slenderobjdet_amd.modeling.meta_arch import FCOSV2, FCOSRepPoints

    assert "FCOSRepPoints" in META_ARCH_REGISTRY
    cfg = fresh_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "fcos", "fcos_R_50_FPN_1x.yaml"))
    over = ["MODEL.META_ARCHITECTURE", "FCOSRepPoints", "MODEL.RESNETS.DEPTH", "18", "MODEL.RESNETS.RES2_OUT_CHANNELS", "64", "MODEL.DEVICE", "cpu"]
    cfg.merge_from_list(over)
    model = build_model(cfg)
    assert type(model) is FCOSRepPoints and isinstance(model, FCOSV2)
    assert model.topk_per_box == 5 and model.last_topk is None and model.last_targets is None and model.last_refine is None
    # the reference head (fcos_rpd_s1_topk.py:505-639): two towers of NUM_CONVS x [conv3x3 + bias, GroupNorm], two DeformConv 3x3 without
    # bias, offsets_init = conv3x3 + conv1x1 to 18, offsets_refine / logits = conv1x1 to 18 / K, centerness = conv3x3 to 1, five Scales
    C, K, n = 256, cfg.MODEL.FCOS.NUM_CLASSES, cfg.MODEL.FCOS.NUM_CONVS
    ref = 2 * n * (9 * C * C + C + 2 * C) + 2 * 9 * C * C + (9 * C * C + C) + (18 * C + 18) + (18 * C + 18) + (K * C + K) + (9 * C + 1) + 5
    assert model.head.num_logical_params() == ref
    assert not hasattr(model.head, "cls_pred") and not hasattr(model.head, "box_pred")
    cfg.merge_from_list(["MODEL.FCOS.NORM_REG_TARGETS", "True"])
    with pytest.raises(NotImplementedError, match="NORM_REG_TARGETS"):
        build_model(cfg)


def test_abi_table_has_the_new_entry_points():
    from slenderobjdet_amd import _C

    assert _C._SIGS["sod_fcos_assign_topk_slender"] == _C._SIGS["sod_fcos_assign_topk"]
    assert len(_C._SIGS["sod_points2ltrb_bwd"]) == len(_C._SIGS["sod_points2bbox_bwd"])
    lib = _C.load()
    for name in ("sod_fcos_assign_topk_slender", "sod_points2ltrb_fwd", "sod_points2ltrb_bwd", "sod_fcos_rpd_refine_targets", "sod_fcos_decode_ltrb",
                 "sod_fcos_rpd_finalize", "sod_level_scale_fwd", "sod_level_scale_bwd"):
        assert hasattr(lib, name)


def test_more_than_4096_boxes_in_an_image_is_an_argument_error():
    """The range check comes before any launch: dummy non-null pointers never reach the device."""
    import ctypes

    from slenderobjdet_amd import _C

    lib = _C.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = ctypes.cast((ctypes.c_int * 1)(4), ctypes.c_void_p)
    args = [p, p, p, 1, 5000, 4097, p, p, 1, one, one, one, 80, 0.4, 0.5, 0, -1, 1, 1, p, p, p, p, p, p, p, None]
    assert lib.sod_fcos_rpd_refine_targets(*args) == -1      # SOD_EARG
