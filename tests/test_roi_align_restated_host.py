"""tests/roi_align_restated.py against the oracle it restates (CPU): the float64 forward equals ``od.roi_align`` and the float64
backward equals autograd through it, for both box forms and sampling ratios 0 and 2, on ROIs of the op-level GPU list (map edges,
samples exactly on a validity cut, sub-pixel and clamped ROIs, zero and negative extents, duplicates).  Both sides are float64 and
differ only in summation order: 1e-12 relative."""
import pytest
import torch

import roi_align_restated as RS
from oracle import detection as od

H, W, C, N = RS.MAP_H, RS.MAP_W, 3, 2
AXIS = ("past_top_left", "past_bottom_right", "outside_right", "first_row_on_minus1", "last_row_on_H", "inside_one_cell",
        "on_pixel_centre", "clamp_00", "clamp_HW", "zero_extent", "zero_width", "negative_extent", "overlap_a", "duplicate_of_overlap_a")
ROTATED = ("angle_0", "angle_90", "angle_-90", "angle_180", "angle_45", "angle_-75", "slender_100x4_37", "slender_4x100_m53",
           "corner_outside", "corner_outside_br", "zero_w", "zero_h", "sub_pixel")


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("sampling_ratio", [0, 2])
@pytest.mark.parametrize("scale", [0.25, 1.0 / 16])
def test_restatement_equals_the_oracle(rotated, sampling_ratio, scale):
    rois, names = (RS.rotated_rois if rotated else RS.axis_rois)(scale)
    pick = [names.index(n) for n in (ROTATED if rotated else AXIS)]
    rois = rois[pick]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    dout = torch.randn(len(rois), C, 7, 7, generator=g, dtype=torch.float64)
    ref = od.roi_align(x, rois.double(), (7, 7), scale, sampling_ratio, rotated)
    (gref,) = torch.autograd.grad(ref, x, dout)
    qs = RS.restate(rois, H, W, (7, 7), scale, sampling_ratio, rotated)
    out = RS.forward(qs, x.detach(), (7, 7))
    dx = RS.backward(qs, dout, (N, C, H, W))
    ferr = (out - ref.detach()).abs().max().item()
    berr = (dx - gref).abs().max().item()
    assert ferr <= 1e-12 * ref.detach().abs().max().item(), ferr
    assert berr <= 1e-12 * gref.abs().max().item(), berr
    # the derived quantities are consistent with the primary ones
    assert torch.equal(RS.abs_forward(qs, x.detach(), (7, 7)) >= out.abs() * (1 - 1e-12), torch.ones_like(out, dtype=torch.bool))
    cc = RS.contrib_count(qs, N, H, W)
    assert cc.shape == (len(rois), N, H, W)
    assert torch.equal((RS.abs_backward(qs, torch.ones_like(dout), (N, C, H, W))[:, 0] > 0), cc.sum(0) > 0)
    for i, q in enumerate(qs):
        assert cc[i].sum().item() == int((q["w"] != 0).sum()) and cc[i, 1 - q["b"]].sum().item() == 0


def test_cut_distance_reports_cuts_and_exempts_only_exact_ones():
    rois, names = RS.axis_rois(0.25)
    q64 = RS.restate(rois, H, W, (7, 7), 0.25, 0, False)
    q32 = RS.restate(rois, H, W, (7, 7), 0.25, 0, False, torch.float32)
    i = names.index("first_row_on_minus1")
    smp, rat, exact = RS.cut_distance(q64[i:i + 1], H, W, 0, also=q32[i:i + 1])
    assert exact == 7 * q64[i]["gw"] + 1 and smp == 1.0        # one sample row on y = -1 and roi_h / PH = 2; the next row is 1 px in
    near = rois[i:i + 1].clone()
    near[0, 2] += 2.0 ** -9                                    # y1 moved by 2^-11 feature px: no longer exact, and far too close
    smp, _, exact = RS.cut_distance(RS.restate(near, H, W, (7, 7), 0.25, 2, False), H, W, 2)
    assert exact == 0 and 0 < smp < 1e-3
    with pytest.raises(AssertionError):
        RS.check_cuts(near, ["near"], RS.restate(near, H, W, (7, 7), 0.25, 2, False),
                      RS.restate(near, H, W, (7, 7), 0.25, 2, False, torch.float32), H, W, 2)
    RS.check_cuts(rois, names, q64, q32, H, W, 0)


def test_an_empty_roi_align_call_is_a_no_op_in_the_c_abi():
    """R = 0: torch gives an empty ROI tensor and the empty output no storage (NULL pointers); the entry points return before any
    launch, so this needs no GPU.  With R > 0 a NULL pointer is still an argument error."""
    from slenderobjdet_amd import _C

    lib = _C.load()
    x = torch.zeros(8)
    for name in ("sod_roi_align_fwd", "sod_roi_align_fwd_f32"):
        assert getattr(lib, name)(x.data_ptr(), None, None, 0, 1, 1, 1, 8, 7, 7, 0.25, 0, 0, None) == 0
        assert getattr(lib, name)(x.data_ptr(), None, x.data_ptr(), 1, 1, 1, 1, 8, 7, 7, 0.25, 0, 0, None) == -1
        assert getattr(lib, name)(x.data_ptr(), x.data_ptr(), None, 1, 1, 1, 1, 8, 7, 7, 0.25, 0, 0, None) == -1
    assert lib.sod_roi_align_bwd(None, None, x.data_ptr(), 0, 1, 1, 1, 8, 7, 7, 0.25, 0, 0, None) == 0
    assert lib.sod_roi_align_bwd(None, x.data_ptr(), x.data_ptr(), 1, 1, 1, 1, 8, 7, 7, 0.25, 0, 0, None) == -1
