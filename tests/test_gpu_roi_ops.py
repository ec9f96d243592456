"""Op-level GPU tests of the two-stage path's operators against float64: ROIAlign forward / backward (the generic kernel, the tiled
fixed-point backward every FPN level uses, the fp32-feature entry point), the RPN clip + filter kernel (bit-exact) and ROIPooler.

ROIAlign bars are assembled per output element from the reference alone (tests/roi_align_restated.py), never from the kernel:

  coordinates   4 * d32, d32 = max |restated(fp32 coordinates) - restated(float64 coordinates)| of the case (per 32-channel chunk in
                the tiled backward), measured on the CPU; the factor covers the device's sinf / cosf differing from the CPU's by a
                few ulp.  The measured d32 is written beside every case below (H x W = 40 x 48, bf16-representable randn features).
  accumulation  (addends + 8) * 2^-24 * (sum of absolute addends); addends = 4 gh gw forward, contribution count backward.
  fixed point   tiled backward only: contrib_count[r, p] * gmax[r, chunk] * 2^-F for each ROI r touching pixel p, F the kernel's
                fraction bits (24 up to 64 bins, 29 - ceil(log2 bins) beyond: csrc/detection_ops.hip roi_bwd_frac_bits; the step is
                2^(ex - F) <= gmax * 2^(1 - F) and every addend is rounded to nearest, half a step at most).

No bar may exceed 1e-4 * max(max|ref|, 1), and no element is left out of a comparison.  ROIAlign is discontinuous where a sample
crosses -1, H or W and (sampling ratio 0) where roi / P crosses an integer: every case asserts (RS.check_cuts) that, restated in
both precisions, nothing lies within 1e-3 of such a cut, except the dyadic quantities RS.ON_A_CUT puts exactly on one."""
import functools
import math

import pytest
import torch

import roi_align_restated as RS
from oracle import detection as od
from oracle import nn as onn
from oracle import rcnn as orc

pytestmark = pytest.mark.gpu

H, W, N = RS.MAP_H, RS.MAP_W, 2
EPS = 2.0 ** -24
CAP = 1e-4
ZERO_DOUT = ("overlap_b", "angle_30")      # the ROI of each list whose dout is all zero


def _g(s):
    return torch.Generator().manual_seed(s)


def frac_bits(nb):
    """csrc/detection_ops.hip roi_bwd_frac_bits, from the comment above roi_align_bwd_tile_kernel."""
    return 24 if nb <= 64 else 29 - math.ceil(math.log2(nb))


@functools.lru_cache(maxsize=None)
def _case(rotated, sr, scale, out_size=(7, 7), pick=None, only_last=False):
    """The ROI list restated once in both precisions, with the discontinuity condition asserted and printed."""
    rois, names = (RS.rotated_rois if rotated else RS.axis_rois)(scale)
    if pick is not None:
        idx = [names.index(n) for n in pick]
        rois, names = rois[idx], [names[i] for i in idx]
    if only_last:
        rois = rois.clone()
        rois[:, 0] = N - 1
    q64 = RS.restate(rois, H, W, out_size, scale, sr, rotated)
    q32 = RS.restate(rois, H, W, out_size, scale, sr, rotated, torch.float32)
    cuts = RS.check_cuts(rois, names, q64, q32, H, W, sr)
    print(f"cut_distance rotated={rotated} sr={sr} scale={scale} out={out_size}: sample {cuts[0]:.4g} ratio {cuts[1]:.4g} exact {cuts[2]}")
    return {"rois": rois, "names": names, "q64": q64, "q32": q32, "out_size": out_size, "scale": scale, "sr": sr, "rotated": rotated}


def _features(C, rounded=True, seed=0):
    x = torch.randn(N, C, H, W, generator=_g(seed))
    return onn.rb(x) if rounded else x


def _dout(case, C, mode, seed=1):
    """(R, C, PH, PW) fp32.  "unit": randn.  "span": per-ROI magnitudes 1e-4 ... 1e3 in one launch.  One ROI's dout is all zero; from
    C = 64 on, the second 32-channel chunk is scaled by 2^-10 (a scale shared between chunks would cost it ten bits)."""
    PH, PW = case["out_size"]
    R = len(case["names"])
    d = torch.randn(R, C, PH, PW, generator=_g(seed))
    if mode == "span":
        mags = torch.tensor([1e-4, 1e3, 1e-2, 30.0, 1.0, 1e2, 1e-3])
        d = d * mags[torch.arange(R) % len(mags)].reshape(R, 1, 1, 1)
    for i, n in enumerate(case["names"]):
        if n in ZERO_DOUT:
            d[i] = 0
    if C >= 64:
        d[:, 32:64] *= 2.0 ** -10
    return d


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _check_fwd(cuda, case, x, label):
    from slenderobjdet_amd.layers import functional as HF

    q64, q32, out_size = case["q64"], case["q32"], case["out_size"]
    xd = x.double()
    ref, r32 = RS.forward(q64, xd, out_size), RS.forward(q32, xd, out_size)
    d32 = (ref - r32).abs().max().item()
    addends = torch.tensor([4.0 * max(q["gh"], 0) * max(q["gw"], 0) for q in q64], dtype=torch.float64).reshape(-1, 1, 1, 1)
    bar = 4 * d32 + (addends + 8) * EPS * RS.abs_forward(q64, xd, out_size)
    assert bar.max().item() <= CAP * max(ref.abs().max().item(), 1.0), (label, bar.max().item())
    out = HF.roi_align_fwd(_nhwc(x).to(cuda).to(HF.ACT_DTYPE), case["rois"].to(cuda), out_size, case["scale"], case["sr"], case["rotated"])
    out = out.cpu().double().permute(0, 3, 1, 2)
    err = (out - ref).abs()
    print(f"{label}: d32 {d32:.3g} max bar {bar.max().item():.3g} max err {err.max().item():.3g} worst err/bar {(err / bar).max().item():.3g}")
    assert bool((err <= bar).all()), (label, err.max().item(), (err / bar).max().item())
    for i, q in enumerate(q64):      # a ROI without a valid sample: exactly zero
        if q["w"].numel() == 0 or not bool(q["valid"].any()):
            assert not bool(out[i].any()), (label, case["names"][i])
    return out


def _bwd_bar(case, dout, C, tiled):
    """-> (ref, bar, d32 of the case, touched (N, H, W) bool)."""
    q64, q32 = case["q64"], case["q32"]
    shape = (N, C, H, W)
    dd = dout.double()
    ref, r32 = RS.backward(q64, dd, shape), RS.backward(q32, dd, shape)
    diff = (ref - r32).abs()
    if tiled:      # per 32-channel chunk: never more than the case's d32
        d32 = diff.reshape(N, C // 32, 32, H, W).amax(dim=(0, 2, 3, 4)).repeat_interleave(32).reshape(1, C, 1, 1)
    else:
        d32 = diff.max()
    cc = torch.maximum(RS.contrib_count(q64, N, H, W), RS.contrib_count(q32, N, H, W))      # (R, N, H, W)
    bar = 4 * d32 + (cc.sum(0)[:, None] + 8) * EPS * RS.abs_backward(q64, dd, shape)
    if tiled:
        PH, PW = case["out_size"]
        gmax = dd.abs().reshape(len(q64), C // 32, -1).amax(dim=2)                          # (R, chunks)
        fixed = torch.einsum("rnhw,rk->nkhw", cc, gmax) * 2.0 ** -frac_bits(PH * PW)
        bar = bar + fixed.repeat_interleave(32, dim=1)
    return ref, bar, diff.max().item(), cc.sum(0) > 0


def _check_bwd(cuda, case, dout, C, label, tiled):
    from slenderobjdet_amd.layers import functional as HF

    assert tiled == (C % 32 == 0)
    ref, bar, d32, touched = _bwd_bar(case, dout, C, tiled)
    assert bar.max().item() <= CAP * max(ref.abs().max().item(), 1.0), (label, bar.max().item(), ref.abs().max().item())
    dx = HF.roi_align_bwd(_nhwc(dout).to(cuda), case["rois"].to(cuda), (N, H, W, C), case["scale"], case["sr"], case["rotated"])
    dx = dx.cpu().double().permute(0, 3, 1, 2)
    err = (dx - ref).abs()
    print(f"{label}: d32 {d32:.3g} max|ref| {ref.abs().max().item():.3g} max bar {bar.max().item():.3g} max err {err.max().item():.3g} "
          f"worst err/bar {(err / bar).max().item():.3g}")
    assert bool((err <= bar).all()), (label, err.max().item(), (err / bar).max().item())
    assert not bool(dx.permute(0, 2, 3, 1)[~touched].any()), label      # a pixel no sample reaches (in either precision) receives nothing
    return dx


# ------------------------------------------------------------------------------------------------ tiled backward (C % 32 == 0)
# measured d32 (CPU, max over the case; max|ref| is 24 / 19.5 / 4.5e3 axis-aligned and 9.7 / 7.6 / 2.5e3 rotated), for
# C = 32 unit / C = 64 unit / C = 64 span; either scale gives the same figure (the ROIs are the same feature-space numbers):
#   axis    sr 0: 1.78e-05 / 2.51e-05 / 6.48e-03    sr 2: 8.35e-06 / 8.96e-06 / 4.70e-03
#   rotated sr 0: 8.14e-06 / 8.83e-06 / 2.41e-03    sr 2: 6.52e-06 / 5.19e-06 / 3.42e-03
@pytest.mark.parametrize("scale", [0.25, 1.0 / 16])
@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("C,mode", [(32, "unit"), (64, "unit"), (64, "span")])
def test_roi_align_tiled_backward(cuda, C, mode, rotated, sr, scale):
    case = _case(rotated, sr, scale)
    _check_bwd(cuda, case, _dout(case, C, mode), C, f"tiled bwd C={C} {mode} rotated={rotated} sr={sr} scale={scale}", tiled=True)


@pytest.mark.parametrize("rotated", [False, True])
def test_roi_align_backward_rois_in_last_image_only(cuda, rotated):
    case = _case(rotated, 0, 0.25, only_last=True)      # d32 1.78e-05 axis-aligned, 8.14e-06 rotated
    dx = _check_bwd(cuda, case, _dout(case, 32, "unit"), 32, f"tiled bwd last image only rotated={rotated}", tiled=True)
    assert not bool(dx[: N - 1].any())


@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("C", [32, 8])
def test_roi_align_rois_without_samples_give_exact_zeros(cuda, C, sr):
    """ROIs entirely outside the map, and (adaptive ratio: ceil(roi / P) <= 0 samples) zero and negative extents: output and gradient
    are exactly zero.  With a fixed sampling ratio a zero or negative extent still takes its samples (aligned=True does not clamp the
    ROI size, oracle/detection.py::roi_align): those are compared in the cases above and below, not here."""
    from slenderobjdet_amd.layers import functional as HF

    for rotated in (False, True):
        pick = ("outside_right", "outside_top_left") + (("zero_extent", "zero_width", "negative_extent") if sr == 0 else ()) if not rotated \
            else (("zero_w", "zero_h") if sr == 0 else ())
        if not pick:
            continue
        case = _case(rotated, sr, 0.25, pick=pick)
        x = _features(C)
        ref = RS.forward(case["q64"], x.double(), (7, 7))
        assert not bool(ref.any())      # the reference says zero; so must the kernels, exactly
        out = HF.roi_align_fwd(_nhwc(x).to(cuda).bfloat16(), case["rois"].to(cuda), (7, 7), 0.25, sr, rotated)
        dx = HF.roi_align_bwd(_nhwc(_dout(case, C, "unit")).to(cuda), case["rois"].to(cuda), (N, H, W, C), 0.25, sr, rotated)
        assert not bool(out.any()) and not bool(dx.any())


# headroom of the fixed point: every bin of a ROI clamped onto pixel (0, 0) lands on that pixel, dout all of one sign with a mantissa
# of 0.9.  The clamped ROI is dyadic and each of its weights exactly 1; the second ROI (inside one pixel cell) is where d32 comes from:
# k = -3: 1.65e-06 (sr 0) 1.24e-06 (sr 2); k = 0: 1.32e-05 9.93e-06; k = 5: 4.23e-04 3.18e-04 (max|ref| 5.5 / 44 / 1.4e3).
@pytest.mark.parametrize("k", [-3, 0, 5])
@pytest.mark.parametrize("sr", [0, 2])
def test_roi_align_tiled_backward_headroom_7x7(cuda, k, sr):
    case = _case(False, sr, 0.25, pick=("clamp_00", "inside_one_cell"))
    dout = torch.full((2, 32, 7, 7), 0.9 * 2.0 ** k)
    dx = _check_bwd(cuda, case, dout, 32, f"headroom 7x7 k={k} sr={sr}", tiled=True)
    assert abs(dx[0, 0, 0, 0].item() / (49 * 0.9 * 2.0 ** k) - 1) < 1e-5


# 196 and 128 bins on one pixel: 24 fraction bits (the scale before roi_bwd_frac_bits) wrap the 32-bit LDS accumulator.
# measured d32: (14, 14) 6.62e-05 (sr 0) 3.16e-05 (sr 2), max|ref| 176; (8, 16) 0 (every coordinate is dyadic), max|ref| 115.
@pytest.mark.parametrize("out_size", [(14, 14), (8, 16)])
@pytest.mark.parametrize("sr", [0, 2])
def test_roi_align_tiled_backward_large_bin_counts(cuda, out_size, sr):
    case = _case(False, sr, 0.25, out_size=out_size, pick=("clamp_00", "inside_one_cell", "overlap_a"))
    dout = torch.full((3, 32) + out_size, 0.9)
    dx = _check_bwd(cuda, case, dout, 32, f"large bins {out_size} sr={sr}", tiled=True)
    assert abs(dx[0, 0, 0, 0].item() / (out_size[0] * out_size[1] * 0.9) - 1) < 1e-5


# ------------------------------------------------------------------------------------------------ generic backward (other C)
# measured d32 for C = 8 / 24 / 40 (max|ref| 8 ... 24):
#   axis    sr 0: 1.00e-05 / 1.66e-05 / 1.58e-05    sr 2: 4.84e-06 / 8.85e-06 / 8.69e-06
#   rotated sr 0: 8.23e-06 / 7.26e-06 / 1.17e-05    sr 2: 4.34e-06 / 5.17e-06 / 7.39e-06
@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("C", [8, 24, 40])
def test_roi_align_generic_backward(cuda, C, rotated, sr):
    case = _case(rotated, sr, 0.25)
    _check_bwd(cuda, case, _dout(case, C, "unit"), C, f"generic bwd C={C} rotated={rotated} sr={sr}", tiled=False)


# ------------------------------------------------------------------------------------------------ forward
# measured d32 for C = 8 / 32 / 256 (either scale; max|ref| 2.3 ... 3.5):
#   axis    sr 0: 4.12e-06 / 5.70e-06 / 1.14e-05    sr 2: 3.56e-06 / 4.39e-06 / 6.74e-06
#   rotated sr 0 and sr 2 alike: 5.45e-06 / 5.91e-06 / 5.55e-06
@pytest.mark.parametrize("scale", [0.25, 1.0 / 16])
@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("C", [8, 32, 256])
def test_roi_align_forward(cuda, C, rotated, sr, scale):
    _check_fwd(cuda, _case(rotated, sr, scale), _features(C), f"fwd C={C} rotated={rotated} sr={sr} scale={scale}")


def _many_rois():
    """56 distinct axis-aligned ROIs: the list above and 36 seeded ones with dyadic feature coordinates."""
    rois, names = RS.axis_rois(0.25)
    g = _g(11)
    lo = torch.stack((torch.randint(-64, 40 * 64, (36,), generator=g), torch.randint(-64, 32 * 64, (36,), generator=g)), 1) / 64.0
    wh = torch.randint(48, 20 * 64, (36, 2), generator=g) / 64.0
    extra = torch.cat((torch.randint(0, N, (36, 1), generator=g).float(), (lo + 0.5) * 4, (lo + wh + 0.5) * 4), 1)
    return torch.cat((rois, extra)), names + [f"seeded{i}" for i in range(36)]


def test_roi_align_forward_second_grid_stride_trip(cuda):
    """R = 1400 at C = 256, (7, 7): R * 49 * 32 work items exceed the launch cap of 8192 * 256, so the grid-stride loop makes a second
    trip.  56 distinct ROIs repeated in a shuffled order: the reference is computed once per distinct ROI.  d32 = 1.16e-05."""
    from slenderobjdet_amd.layers import functional as HF

    C, R = 256, 1400
    assert R * 49 * (C // 8) > 8192 * 256
    rois, names = _many_rois()
    q64 = RS.restate(rois, H, W, (7, 7), 0.25, 0, False)
    q32 = RS.restate(rois, H, W, (7, 7), 0.25, 0, False, torch.float32)
    cuts = RS.check_cuts(rois, names, q64, q32, H, W, 0)
    print("cut_distance second trip:", cuts)
    x = _features(C)
    xd = x.double()
    ref, r32 = RS.forward(q64, xd, (7, 7)), RS.forward(q32, xd, (7, 7))
    d32 = (ref - r32).abs().max().item()
    addends = torch.tensor([4.0 * max(q["gh"], 0) * max(q["gw"], 0) for q in q64], dtype=torch.float64).reshape(-1, 1, 1, 1)
    bar = 4 * d32 + (addends + 8) * EPS * RS.abs_forward(q64, xd, (7, 7))
    assert bar.max().item() <= CAP * max(ref.abs().max().item(), 1.0)
    order = torch.cat([torch.randperm(len(rois), generator=_g(12)) for _ in range(R // len(rois))])
    assert len(order) == R
    xg = _nhwc(x).to(cuda).bfloat16()
    out = HF.roi_align_fwd(xg, rois[order].to(cuda), (7, 7), 0.25, 0, False).cpu().double().permute(0, 3, 1, 2)
    err = (out - ref[order]).abs()
    print(f"fwd second trip: d32 {d32:.3g} max bar {bar.max().item():.3g} max err {err.max().item():.3g} worst err/bar {(err / bar[order]).max().item():.3g}")
    assert bool((err <= bar[order]).all())
    assert HF.roi_align_fwd(xg, rois[:0].to(cuda), (7, 7), 0.25, 0, False).shape == (0, 7, 7, C)
    one = HF.roi_align_fwd(xg, rois[:1].to(cuda), (7, 7), 0.25, 0, False).cpu().double().permute(0, 3, 1, 2)
    assert bool(((one - ref[:1]).abs() <= bar[:1]).all())


# ------------------------------------------------------------------------------------------------ fp32-feature entry point
@pytest.fixture()
def f32mode():
    from slenderobjdet_amd.layers import functional as HF

    prev = HF.set_precision("fp32")
    yield HF
    HF.set_precision(prev)


# measured d32 (unrounded fp32 features) for C = 8 / 64: axis sr 0 3.78e-06 / 6.37e-06, sr 2 3.81e-06 / 4.02e-06;
# rotated (both ratios) 4.29e-06 / 5.68e-06
@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("C", [8, 64])
def test_roi_align_forward_f32_features(cuda, f32mode, C, rotated, sr):
    assert f32mode.is_f32()
    _check_fwd(cuda, _case(rotated, sr, 0.25), _features(C, rounded=False, seed=5), f"fwd f32 C={C} rotated={rotated} sr={sr}")


def test_roi_align_tiled_backward_in_f32_mode(cuda, f32mode):
    case = _case(True, 0, 0.25)      # d32 8.83e-06
    _check_bwd(cuda, case, _dout(case, 64, "unit"), 64, "tiled bwd in f32 mode", tiled=True)


# ------------------------------------------------------------------------------------------------ sod_rpn_clip_filter
IMAGE_HW = ((200.0, 300.0), (128.5, 257.25), (64.0, 48.0))
NEXT_ABOVE_1 = 1.0000001192092896      # nextafter(1, 2) in fp32
ABOVE_1_AFTER_NORMALISING = 1.0000152587890625      # 181 + ulp(181) - 180: the smallest angle above 1 that (a + 180) % 360 - 180 keeps above 1


def _clip_inputs(D, h, w, seed):
    M = 300
    g = _g(seed)
    if D == 4:
        xy = torch.rand(M, 2, generator=g) * torch.tensor([w + 60.0, h + 60.0]) - 30.0
        b = torch.cat((xy, xy + torch.rand(M, 2, generator=g) * 80.0), 1)
        special = [
            [-20.0, 10.0, 15.0, 30.0], [w - 10.0, 10.0, w + 25.0, 30.0], [10.0, -12.0, 30.0, 9.0], [10.0, h - 7.0, 30.0, h + 11.0],      # over each edge
            [-40.0, 10.0, -5.0, 30.0], [w + 5.0, 10.0, w + 40.0, 30.0], [10.0, -30.0, 30.0, -2.0], [10.0, h + 1.0, 30.0, h + 9.0],        # outside: zero width
            [-50.0, -50.0, -10.0, -10.0], [w + 1.0, h + 1.0, w + 9.0, h + 9.0],
            [10.0, 10.0, 14.0, 30.0], [10.0, 10.0, 30.0, 14.0], [-6.0, 10.0, 4.0, 30.0], [10.0, h - 4.0, 30.0, h + 8.0],                 # side == 4 (after clipping)
            [10.0, 10.0, 14.5, 30.0], [10.0, 10.0, 10.0, 30.0], [10.0, 10.0, 30.0, 10.0], [-30.0, -30.0, w + 30.0, h + 30.0],
        ]
    else:
        ctr = torch.rand(M, 2, generator=g) * torch.tensor([w + 40.0, h + 40.0]) - 20.0
        b = torch.cat((ctr, torch.rand(M, 2, generator=g) * 60.0, torch.rand(M, 1, generator=g) * 1440.0 - 720.0), 1)
        b[::3, 4] = torch.rand(len(b[::3]), generator=g) * 4.0 - 2.0 + 360.0 * torch.randint(-2, 3, (len(b[::3]),), generator=g)      # around the 1-degree rule
        special = [[w - 5.0, 20.0, 40.0, 20.0, a] for a in (180.0, -180.0, 540.0, -540.0, 179.99998, 361.0, -361.0, 1.0, -1.0, NEXT_ABOVE_1,
                                                             -NEXT_ABOVE_1, ABOVE_1_AFTER_NORMALISING, -ABOVE_1_AFTER_NORMALISING, 0.0, 359.5, -359.5)]
        special += [
            [w - 5.0, 20.0, 40.0, 20.0, 0.5], [w - 5.0, 20.0, 40.0, 20.0, 30.0], [3.0, h - 2.0, 20.0, 30.0, -0.75], [3.0, h - 2.0, 20.0, 30.0, 80.0],
            [20.0, 20.0, 4.0, 30.0, 45.0], [20.0, 20.0, 30.0, 4.0, 45.0], [20.0, 20.0, 4.5, 30.0, 45.0], [2.0, 20.0, 8.0, 30.0, 0.0],      # side == 4 (the last: after clipping)
            [20.0, 20.0, 0.0, 30.0, 10.0], [20.0, 20.0, 30.0, 0.0, 0.0], [-60.0, 20.0, 40.0, 20.0, 0.25], [w + 100.0, h + 100.0, 40.0, 20.0, -0.25],
        ]
    sp = torch.tensor(special, dtype=torch.float32)
    b[: len(sp)] = sp
    s = torch.randn(M, generator=g)
    # non-finite: every box field and the score, each of NaN / +inf / -inf; a slot whose score was already -inf
    k = len(sp)
    for f in range(D + 1):
        for v in (float("nan"), float("inf"), float("-inf")):
            if f < D:
                b[k, f] = v
            else:
                s[k] = v
            k += 1
    b[k, 0] = float("nan"); s[k] = float("-inf"); k += 1
    s[k + 5] = float("-inf")      # already empty, box finite
    return b, s


@pytest.mark.parametrize("min_size", [0.0, 4.0])
@pytest.mark.parametrize("D", [4, 5])
def test_rpn_clip_filter_bit_exact(cuda, D, min_size):
    """Against oracle/rcnn.py clip_boxes + nonempty in float32: the kernel's operations are individually rounded fp32 operations in the
    same order (no contraction: halving is exact), so boxes, the -inf pattern of the scores and the bad counter are compared exactly.
    Note on the 1-degree rule: (a + 180) % 360 - 180 in fp32 maps nextafter(1) to exactly 1 (181 + 1.2e-7 rounds to 181), so that box IS
    clipped, in the oracle and in detectron2 alike; the smallest angle the rule leaves alone is 1.0000153."""
    from slenderobjdet_amd.layers import functional as HF

    parts = [_clip_inputs(D, h, w, 20 + i) for i, (h, w) in enumerate(IMAGE_HW)]
    boxes, scores = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
    exp_b, exp_s, bad = boxes.clone(), scores.clone(), 0
    for i, hw in enumerate(IMAGE_HW):
        fin = torch.isfinite(boxes[i]).all(dim=1) & torch.isfinite(scores[i])
        bad += int((~fin).sum())
        clipped = orc.clip_boxes(boxes[i], hw)
        assert clipped.dtype == torch.float32
        exp_b[i][fin] = clipped[fin]
        exp_s[i][~(fin & orc.nonempty(clipped, min_size))] = float("-inf")
    assert bad == 3 * (3 * (D + 1) + 2)      # per image: 3 values x (D fields + score), the NaN box with a -inf score, the -inf score alone
    if D == 5:      # what the cases are there for, stated on the reference
        w = IMAGE_HW[0][1]
        e = exp_b[0]
        assert e[5, 4] == 1.0 and e[6, 4] == -1.0 and e[5, 2] < 40.0 and e[6, 2] < 40.0                  # 361 / -361 normalise to +-1: clipped
        assert e[9, 4] == 1.0 and e[9, 2] < 40.0                                                          # nextafter(1): see the docstring
        assert e[11, 4] > 1.0 and e[11, 2] == 40.0 and e[12, 4] < -1.0 and e[12, 2] == 40.0               # not clipped
        assert e[16].tolist() == [w - 12.5, 20.0, 25.0, 20.0, 0.5] and e[17].tolist() == [w - 5.0, 20.0, 40.0, 20.0, 30.0]
        assert e[0, 4] == -180.0 and e[2, 4] == -180.0 and e[3, 4] == -180.0
    gb, gs = boxes.to(cuda), scores.to(cuda)
    hw = torch.tensor(IMAGE_HW, dtype=torch.float32, device=cuda)
    got_bad = HF.rpn_clip_filter(gb, gs, hw, min_size)
    assert int(got_bad.item()) == bad
    gb, gs = gb.cpu(), gs.cpu()
    assert torch.equal(gs, exp_s)
    finite = torch.isfinite(boxes).all(dim=2)
    assert torch.equal(gb[finite], exp_b[finite])
    assert torch.equal(gb.view(torch.int32), exp_b.view(torch.int32))      # the non-finite rows are left as they were, -0.0 / NaN payloads included
    kept = torch.isfinite(exp_s)
    assert 0.3 < kept.float().mean().item() < 0.95


# ------------------------------------------------------------------------------------------------ ROIPooler
PYR_SCALES = (1 / 4, 1 / 8, 1 / 16, 1 / 32)
PYR_MAPS = ((48, 64), (24, 32), (12, 16), (6, 8))
PC = 32


def _pool_boxes(rotated, which):
    """Per image a list of boxes whose sqrt(area) is exactly 112, 224, 448 (fp32 and float64 agree on the level), 1 % to either side
    of each, 8 (far below: clamps to level 0) and 1000 (far above: clamps to the last), interleaved so that every level's ROIs are
    scattered through the list.  "no_l2": the sizes of level 2 (224 <= s < 448) left out.
    The square boxes of size 112 * 2^k have roi / 7 = 4 exactly, in both precisions: the one quantity here that sits on a cut."""
    sizes = [112.0, 448.0 * 1.01, 8.0, 224.0 * 0.99, 448.0, 112.0 * 0.99, 1000.0, 224.0, 112.0 * 1.01, 448.0 * 0.99, 224.0 * 1.01, 40.0]
    if which == "no_l2":
        sizes = [s for s in sizes if not 224.0 <= s < 448.0]
    if which == "small":      # for the single-level pyramid: everything is pooled from the 1/4 map
        sizes = [112.0, 8.0, 150.0, 40.0, 112.0 * 0.99]
    imgs = []
    for n in range(N):
        rows = []
        for i, s in enumerate(sizes):
            cx, cy = 70.28125 + 9.40625 * i + 20.5 * n, 60.71875 + 7.15625 * i - 11.25 * n
            if rotated:
                rows.append([cx, cy, s / 2, s * 2, (-75.0, 33.0, 0.0, 45.0, 90.0, -20.0)[(i + n) % 6]])      # sqrt(s/2 * 2s) = s
            else:
                rows.append([cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2])
        imgs.append(torch.tensor(rows, dtype=torch.float32))
    return imgs


def _restate_pool(rois, lv, sr, rotated, levels):
    """Per level: (indices, q64, q32) with the discontinuity condition asserted."""
    per = []
    for l in range(levels):
        idx = torch.nonzero(lv == l).squeeze(1)
        Hl, Wl = PYR_MAPS[l]
        q64 = RS.restate(rois[idx], Hl, Wl, (7, 7), PYR_SCALES[l], sr, rotated)
        q32 = RS.restate(rois[idx], Hl, Wl, (7, 7), PYR_SCALES[l], sr, rotated, torch.float32)
        cuts = RS.check_cuts(rois[idx], [f"level{l}_{int(i)}" for i in idx], q64, q32, Hl, Wl, sr, exact_ok=True)
        print(f"pooler cut_distance level {l} ({len(idx)} rois):", cuts)
        per.append((idx, q64, q32))
    return per


@functools.lru_cache(maxsize=None)
def _pool_reference(rotated, which, levels):
    sr = 0
    boxes = _pool_boxes(rotated, which)
    rois = torch.cat([torch.cat((torch.full((len(b), 1), float(n)), b), 1) for n, b in enumerate(boxes)])
    feats = [onn.rb(torch.randn(N, PC, h, w, generator=_g(30 + l))) for l, (h, w) in enumerate(PYR_MAPS[:levels])]
    fd = [f.double().requires_grad_(True) for f in feats]
    ref = orc.roi_pool(fd, rois.double(), list(PYR_SCALES[:levels]), 7, sr)
    wgt = onn.rb(torch.randn(ref.shape, generator=_g(40)))      # the pooler's output is bf16, and so is the gradient autograd hands back
    gref = torch.autograd.grad((ref * wgt.double()).sum(), fd, allow_unused=True)      # a level without ROIs is not in the graph
    gref = [torch.zeros_like(f) if g is None else g for g, f in zip(gref, fd)]
    D = rois.shape[1] - 1
    areas = rois[:, 3] * rois[:, 4] if D == 5 else (rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2])
    lv = orc.assign_levels(areas.double(), 2, 1 + levels) if levels > 1 else torch.zeros(len(rois), dtype=torch.long)
    per = _restate_pool(rois, lv, sr, rotated, levels)
    fbar = torch.zeros_like(ref)
    gbars = []
    for l, (idx, q64, q32) in enumerate(per):
        xd = feats[l].double()
        r64 = RS.forward(q64, xd, (7, 7))
        assert (r64 - ref.detach()[idx]).abs().max().item() <= 1e-12 * max(ref.abs().max().item(), 1.0) if len(idx) else True
        d32 = (r64 - RS.forward(q32, xd, (7, 7))).abs().max().item() if len(idx) else 0.0
        addends = torch.tensor([4.0 * max(q["gh"], 0) * max(q["gw"], 0) for q in q64], dtype=torch.float64).reshape(-1, 1, 1, 1)
        fb = 4 * d32 + (addends + 8) * EPS * RS.abs_forward(q64, xd, (7, 7))
        assert len(idx) == 0 or fb.max().item() <= CAP * max(r64.abs().max().item(), 1.0)
        fbar[idx] = fb
        # backward: the tiled bar of this level's launch
        Hl, Wl = PYR_MAPS[l]
        dd = wgt[idx].double()
        shape = (N, PC, Hl, Wl)
        b64, b32 = RS.backward(q64, dd, shape), RS.backward(q32, dd, shape)
        assert (b64 - gref[l]).abs().max().item() <= 1e-12 * max(gref[l].abs().max().item(), 1.0)
        cc = torch.maximum(RS.contrib_count(q64, N, Hl, Wl), RS.contrib_count(q32, N, Hl, Wl))
        gb = 4 * (b64 - b32).abs().max() + (cc.sum(0)[:, None] + 8) * EPS * RS.abs_backward(q64, dd, shape)
        if len(idx):
            gb = gb + torch.einsum("rnhw,r->nhw", cc, dd.abs().reshape(len(idx), -1).amax(dim=1))[:, None] * 2.0 ** -24
            assert gb.max().item() <= CAP * max(b64.abs().max().item(), 1.0)
        print(f"pooler level {l}: fwd d32 {d32:.3g} bwd d32 {(b64 - b32).abs().max().item():.3g}")
        gbars.append(gb)
    return {"boxes": boxes, "rois": rois, "feats": feats, "ref": ref.detach(), "wgt": wgt, "gref": gref, "lv": lv, "fbar": fbar, "gbars": gbars}


# measured d32 per level 0..3 of the four-level list, forward / backward:
#   ROIAlignV2      7.47e-06 3.14e-06 2.07e-06 1.01e-06 / 8.94e-06 2.21e-06 1.65e-06 9.32e-07
#   ROIAlignRotated 6.43e-06 3.48e-06 9.82e-07 6.44e-07 / 5.79e-06 1.81e-06 8.32e-07 6.86e-07
# single level: ROIAlignV2 5.49e-06 / 8.58e-06, ROIAlignRotated 5.87e-06 / 7.18e-06  (all far below the bf16 step of the output)
@pytest.mark.parametrize("which,levels", [("all", 4), ("no_l2", 4), ("small", 1)])
@pytest.mark.parametrize("pooler_type", ["ROIAlignV2", "ROIAlignRotated"])
def test_roi_pooler_forward_backward(cuda, pooler_type, which, levels):
    from slenderobjdet_amd.layers import nn as hnn
    from slenderobjdet_amd.modeling.roi_heads.roi_heads import ROIPooler
    from slenderobjdet_amd.structures import Boxes, RotatedBoxes

    assert od.ROI_ALIGN_IMPL == "loop" and hnn.GradPark.current is None
    rotated = pooler_type == "ROIAlignRotated"
    R = _pool_reference(rotated, which, levels)
    pooler = ROIPooler(7, list(PYR_SCALES[:levels]), 0, pooler_type)
    cls = RotatedBoxes if rotated else Boxes
    box_lists = [cls(b.to(cuda)) for b in R["boxes"]]
    lv = R["lv"]
    if levels > 1:
        got_lv = pooler.assign_levels(torch.cat([b.area() for b in box_lists])).cpu()
        assert torch.equal(got_lv, lv)
        counts = torch.bincount(lv, minlength=levels).tolist()
        assert (counts[2] == 0) == (which == "no_l2") and all(c > 0 for i, c in enumerate(counts) if i != 2)
        for l in set(lv.tolist()):      # every level's ROIs are scattered through the list: other levels' lie between them
            idx = torch.nonzero(lv == l).squeeze(1)
            assert int(idx.max() - idx.min()) + 1 > len(idx) > 1
    feats = [_nhwc(f).to(cuda).bfloat16().requires_grad_(True) for f in R["feats"]]
    out = pooler(feats, box_lists)
    assert out.dtype == torch.bfloat16 and out.shape == (len(lv), 7, 7, PC)
    ref = R["ref"]
    err = (out.detach().cpu().double().permute(0, 3, 1, 2) - ref).abs()      # rows in input order
    bar = R["fbar"] + 2.0 ** -7 * ref.abs()
    print(f"pooler {pooler_type} {which} L={levels}: fwd max err {err.max().item():.3g} worst err/bar {(err / bar).max().item():.3g}")
    assert bool((err <= bar).all())
    grads = torch.autograd.grad((out.float() * _nhwc(R["wgt"]).to(cuda)).sum(), feats)
    for l, g in enumerate(grads):
        gref = R["gref"][l]
        g = g.cpu().double().permute(0, 3, 1, 2)
        assert g.shape == gref.shape
        gerr = (g - gref).abs()
        gbar = R["gbars"][l] + 2.0 ** -7 * gref.abs()
        print(f"   level {l}: bwd max|ref| {gref.abs().max().item():.3g} max err {gerr.max().item():.3g} worst err/bar {(gerr / gbar).max().item():.3g}")
        assert bool((gerr <= gbar).all()), l
        if int((lv == l).sum()) == 0:
            assert not bool(g.any())      # the empty level's gradient is exactly zero
