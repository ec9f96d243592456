"""FCOSTopK, host side (CPU): the restatement (tests/fcos_topk_restated.py) against the fixtures the reference's own Python produced
(tests/golden/fcos_topk/, generator make_golden_fcos_topk.py), the registry entry, and the C-ABI table.  The kernels themselves are
checked against the same fixtures and the same restatement in tests/test_gpu_fcos_topk.py."""
import os

import numpy as np
import pytest
import torch

import fcos_topk_restated as RS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_topk")
TARGET_FILES = ("targets_seed1.npz", "targets_seed2.npz")
LOSS_FILES = ("losses_giou.npz", "losses_iou.npz")


def load_gts(z):
    n = len([k for k in z.files if k.startswith("boxes")])
    return [torch.from_numpy(z[f"boxes{i}"]) for i in range(n)], [torch.from_numpy(z[f"classes{i}"]) for i in range(n)]


@pytest.mark.parametrize("name", TARGET_FILES)
@pytest.mark.parametrize("radius", [1.5, 0.0])
def test_restated_targets_equal_the_reference(name, radius):
    z = np.load(os.path.join(GOLD, name))
    boxes, classes = load_gts(z)
    hw = [tuple(int(v) for v in r) for r in z["level_hw"]]
    lab, reg, _ctr, idx, sel = RS.topk_targets(hw, z["strides"].tolist(), boxes, classes, radius, int(z["num_classes"]))
    assert torch.equal(lab, torch.from_numpy(z[f"gt_classes_r{radius}"]))
    assert torch.equal(reg, torch.from_numpy(z[f"reg_targets_r{radius}"]))
    ref = torch.from_numpy(z[f"topk_locations_r{radius}"])
    assert torch.equal(sel, ref)
    fg = lab != int(z["num_classes"])
    assert int(z[f"num_gt_over_topk_r{radius}"]) >= 2 and 0 < int(sel.sum()) < int(fg.sum())      # the cut is exercised
    assert bool((sel <= fg).all()) and bool(((idx >= 0) == fg).all())


@pytest.mark.parametrize("name", LOSS_FILES)
def test_restated_losses_equal_the_reference(name):
    z = np.load(os.path.join(GOLD, name))
    boxes, classes = load_gts(z)
    hw = [tuple(int(v) for v in r) for r in z["level_hw"]]
    K = int(z["num_classes"])
    lab, reg, _ctr, _idx, sel = RS.topk_targets(hw, z["strides"].tolist(), boxes, classes, float(z["radius"]), K)
    assert torch.equal(lab, torch.from_numpy(z["gt_classes"])) and torch.equal(sel, torch.from_numpy(z["topk_locations"]))
    nl = len(hw)
    preds = [[torch.from_numpy(z[f"{k}{l}"]).clone().requires_grad_(True) for l in range(nl)] for k in ("logits", "box_reg", "ctrness")]
    cls, box, ctr = RS.permute_and_concat(preds[0], preds[1], preds[2], K)
    out = RS.topk_losses(lab.reshape(-1), reg.reshape(-1, 4), sel.reshape(-1), cls, box, ctr, K, float(z["alpha"]), float(z["gamma"]),
                         name[len("losses_"):-len(".npz")])
    for k, v in out.items():
        ref = float(z["loss::" + k])
        assert abs(float(v.detach()) - ref) <= 1e-5 * max(abs(ref), 1.0), (k, float(v.detach()), ref)
    grads = torch.autograd.grad(sum(out.values()), preds[0] + preds[1] + preds[2])
    names = [f"grad_{k}{l}" for k in ("logits", "box_reg", "ctrness") for l in range(nl)]
    for n, g in zip(names, grads):
        ref = torch.from_numpy(z[n])
        assert float((g - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1.0), n


def test_tie_at_the_cut_takes_the_lower_location():
    """Box (8, 8, 40, 40), radius 0: 16 positives on the stride-8 level with centerness 4 x 0.6, 8 x 0.2928, 4 x 0.1429.  The rule picks the
    four 0.6 and the lowest-index 0.2928."""
    hw, strides = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)], [8, 16, 32, 64, 128]
    lab, _reg, ctr, _idx, sel = RS.topk_targets(hw, strides, [torch.tensor([[8.0, 8.0, 40.0, 40.0]])], [torch.tensor([3])], 0.0, 80)
    pos = (lab[0] != 80).nonzero().squeeze(1)
    assert pos.numel() == 16 and int(pos.max()) < 16 * 20
    vals = ctr[0, pos]
    assert sorted(round(float(v), 4) for v in vals) == [0.1429] * 4 + [0.2928] * 8 + [0.6] * 4
    mid = pos[(vals > 0.2) & (vals < 0.5)]
    picked = sel[0].nonzero().squeeze(1)
    assert picked.numel() == 5
    assert set(picked.tolist()) == set(pos[vals > 0.5].tolist()) | {int(mid.min())}


def test_build_model_resolves_fcos_topk():
    from slenderobjdet_amd.config import fresh_cfg
    from slenderobjdet_amd.modeling import META_ARCH_REGISTRY, build_model
    from slenderobjdet_amd.modeling.meta_arch import FCOSTopK, FCOSV2

    assert "FCOSTopK" in META_ARCH_REGISTRY
    cfg = fresh_cfg()
    cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(GOLD))), "configs", "fcos", "fcos_R_50_FPN_1x.yaml"))
    cfg.merge_from_list(["MODEL.META_ARCHITECTURE", "FCOSTopK", "MODEL.RESNETS.DEPTH", "18", "MODEL.RESNETS.RES2_OUT_CHANNELS", "64", "MODEL.DEVICE", "cpu"])
    model = build_model(cfg)
    assert type(model) is FCOSTopK and isinstance(model, FCOSV2)
    assert model.topk_per_box == 5 and model.last_topk is None
    assert type(model).inference is FCOSV2.inference and type(model).prefetch is FCOSV2.prefetch


def test_abi_table_has_the_new_entry_points():
    from slenderobjdet_amd import _C

    n = len(_C._SIGS["sod_fcos_assign"])
    assert len(_C._SIGS["sod_fcos_assign_topk"]) == n + 3              # topk, gt_index, sel
    for base, sel in (("sod_fcos_regctr_loss_fwd", "sod_fcos_regctr_loss_sel_fwd"), ("sod_fcos_regctr_loss_bwd", "sod_fcos_regctr_loss_sel_bwd"),
                      ("sod_fcos_regctr_loss_bwd_f32", "sod_fcos_regctr_loss_sel_bwd_f32")):
        assert len(_C._SIGS[sel]) == len(_C._SIGS[base]) + 1, sel
    lib = _C.load()
    for name in ("sod_fcos_assign_topk", "sod_fcos_regctr_loss_sel_fwd", "sod_fcos_regctr_loss_sel_bwd", "sod_fcos_regctr_loss_sel_bwd_f32"):
        assert hasattr(lib, name)


@pytest.mark.parametrize("topk", [0, 9])
def test_topk_out_of_range_is_an_argument_error(topk):
    """The range check comes before any launch: dummy non-null pointers never reach the device."""
    import ctypes

    from slenderobjdet_amd import _C

    lib = _C.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ints = (ctypes.c_int * 1)(4)
    strides = (ctypes.c_int * 1)(8)
    lo, hi = (ctypes.c_float * 1)(-1.0), (ctypes.c_float * 1)(1e8)
    args = [p, p, p, 1, 1, ctypes.cast(ints, ctypes.c_void_p), ctypes.cast(ints, ctypes.c_void_p), ctypes.cast(strides, ctypes.c_void_p),
            ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(hi, ctypes.c_void_p), 1.5, 80, topk, p, p, p, p, p, p, p, None]
    assert lib.sod_fcos_assign_topk(*args) == -1      # SOD_EARG
