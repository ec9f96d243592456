"""A float64 restatement of ROIAlign(aligned=True) / ROIAlignRotated for the op-level tests, CPU only.

One vectorised function, :func:`restate`, turns (ROIs, map size, output size, scale, sampling ratio) into the per-ROI quantities the
operator is made of: sample positions, validity flags, the four corner indices and weights, and the sample count.  Everything else
(forward, backward, the sums of absolute addends, the per-pixel contribution counts, the distance from the discontinuities) is
derived from those, so a test can state its error bars from the reference alone.  It follows ``oracle/detection.py::roi_align``
operation by operation; ``coord_dtype=torch.float32`` evaluates the same expressions with every operation rounded to fp32 in the
order the HIP kernels use (csrc/detection_ops.hip: roi_align_kernel), which measures what fp32 coordinates alone cost.

tests/test_roi_align_restated_host.py pins the float64 form to ``od.roi_align`` and to autograd through it.
"""
import math

import torch

PI_F32 = 3.14159265358979323846      # the kernel's literal (rounded to fp32 there: the float32 path rounds it the same way)


def restate(rois, H, W, output_size, scale, sampling_ratio=0, rotated=False, coord_dtype=torch.float64):
    """rois (R, 5) [batch, x1, y1, x2, y2] or (R, 6) [batch, cx, cy, w, h, angle_deg].  Returns one dict per ROI:

    ``b`` batch index; ``gh, gw`` samples per bin side; ``count`` = max(gh * gw, 1); ``ratio_h, ratio_w`` = roi_h / PH, roi_w / PW
    (what the adaptive sampling ratio is the ceiling of); ``y, x`` (PH * gh, PW * gw) float64 sample positions before clamping;
    ``valid`` same shape, bool; ``idx`` (4, PH * gh, PW * gw) int64 flat pixel index y * W + x of the corners (yl,xl), (yl,xh),
    (yh,xl), (yh,xh); ``w`` (4, ...) float64 corner weights (zero where not valid).  All arithmetic in ``coord_dtype``.
    """
    PH, PW = output_size
    dt = coord_dtype
    out = []
    r = rois.to(dt)
    s = torch.tensor(scale, dtype=dt)
    half, two = torch.tensor(0.5, dtype=dt), torch.tensor(2.0, dtype=dt)
    for i in range(rois.shape[0]):
        b = int(rois[i, 0])
        if rotated:
            cw, ch = r[i, 1] * s - half, r[i, 2] * s - half
            rw, rh = r[i, 3] * s, r[i, 4] * s
            th = r[i, 5] * torch.tensor(math.pi if dt == torch.float64 else PI_F32, dtype=dt) / torch.tensor(180.0, dtype=dt)
            ct, st = torch.cos(th), torch.sin(th)
            sh, sw = -rh / two, -rw / two
        else:
            sw, sh = r[i, 1] * s - half, r[i, 2] * s - half
            rw, rh = r[i, 3] * s - half - sw, r[i, 4] * s - half - sh
        bh, bw = rh / PH, rw / PW
        gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(bh)))
        gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(bw)))
        q = {"b": b, "gh": gh, "gw": gw, "count": max(gh * gw, 1), "ratio_h": float(bh), "ratio_w": float(bw)}
        nh, nw = PH * max(gh, 0), PW * max(gw, 0)
        if gh <= 0 or gw <= 0:
            nh = nw = 0
        ph = torch.arange(PH, dtype=dt).repeat_interleave(max(gh, 0))[:nh]
        iy = torch.arange(max(gh, 0), dtype=dt).repeat(PH)[:nh]
        pw = torch.arange(PW, dtype=dt).repeat_interleave(max(gw, 0))[:nw]
        ix = torch.arange(max(gw, 0), dtype=dt).repeat(PW)[:nw]
        yy = (sh + ph * bh + (iy + half) * bh / max(gh, 1))[:, None]
        xx = (sw + pw * bw + (ix + half) * bw / max(gw, 1))[None, :]
        if rotated:
            y, x = yy * ct - xx * st + ch, yy * st + xx * ct + cw
        else:
            y, x = yy.expand(nh, nw), xx.expand(nh, nw)
        q["y"], q["x"] = y.double().clone(), x.double().clone()
        valid = ~((y < -1.0) | (y > H) | (x < -1.0) | (x > W))
        y, x = y.clamp(min=0.0), x.clamp(min=0.0)
        yl, xl = y.floor().long(), x.floor().long()
        top, right = yl >= H - 1, xl >= W - 1
        yl, xl = torch.where(top, torch.full_like(yl, H - 1), yl), torch.where(right, torch.full_like(xl, W - 1), xl)
        yh, xh = torch.where(top, yl, yl + 1), torch.where(right, xl, xl + 1)
        y, x = torch.where(top, yl.to(dt), y), torch.where(right, xl.to(dt), x)
        ly, lx = y - yl.to(dt), x - xl.to(dt)
        hy, hx = 1.0 - ly, 1.0 - lx
        q["valid"] = valid
        q["idx"] = torch.stack((yl * W + xl, yl * W + xh, yh * W + xl, yh * W + xh))
        q["w"] = torch.stack((hy * hx, hy * lx, ly * hx, ly * lx)).double() * valid.double()
        out.append(q)
    return out


def _geom(q, output_size):
    PH, PW = output_size
    if q["gh"] <= 0 or q["gw"] <= 0:      # no samples: the ROI's output and gradient are zero
        return PH, 0, PW, 0
    return PH, q["gh"], PW, q["gw"]


def forward(qs, x, output_size):
    """x (N, C, H, W) float64 -> (R, C, PH, PW): gather the corners, weight, average per bin."""
    N, C, H, W = x.shape
    PH, PW = output_size
    out = torch.zeros(len(qs), C, PH, PW, dtype=torch.float64)
    flat = x.double().reshape(N, C, H * W)
    for r, q in enumerate(qs):
        _, gh, _, gw = _geom(q, output_size)
        if gh * gw == 0:
            continue
        acc = torch.zeros(C, PH * gh * PW * gw, dtype=torch.float64)
        for k in range(4):
            acc += flat[q["b"]][:, q["idx"][k].reshape(-1)] * q["w"][k].reshape(1, -1)
        out[r] = acc.reshape(C, PH, gh, PW, gw).sum(dim=(2, 4)) / q["count"]
    return out


def backward(qs, dout, x_shape):
    """dout (R, C, PH, PW) float64 -> dx (N, C, H, W): index_add_ of dout * w / count."""
    N, C, H, W = x_shape
    PH, PW = dout.shape[2:]
    dx = torch.zeros(N, C, H * W, dtype=torch.float64)
    for r, q in enumerate(qs):
        _, gh, _, gw = _geom(q, (PH, PW))
        if gh * gw == 0:
            continue
        g = (dout[r].double() / q["count"])[:, :, None, :, None].expand(C, PH, gh, PW, gw).reshape(C, -1)
        for k in range(4):
            dx[q["b"]].index_add_(1, q["idx"][k].reshape(-1), g * q["w"][k].reshape(1, -1))
    return dx.reshape(N, C, H, W)


def abs_forward(qs, x, output_size):
    """Sum of the absolute addends of every forward output element (the weights are non-negative)."""
    return forward(qs, x.abs(), output_size)


def abs_backward(qs, dout, x_shape):
    """Sum of the absolute addends of every gradient element."""
    return backward(qs, dout.abs(), x_shape)


def contrib_count(qs, N, H, W):
    """(R, N, H, W) float64: per (ROI, pixel), the number of corner contributions with a non-zero weight."""
    cc = torch.zeros(len(qs), N, H * W, dtype=torch.float64)
    for r, q in enumerate(qs):
        if q["w"].numel():
            cc[r, q["b"]].index_add_(0, q["idx"].reshape(-1), (q["w"].reshape(-1) != 0).double())
    return cc.reshape(len(qs), N, H, W)


def cut_distance(qs, H, W, sampling_ratio, also=None):
    """How far the case stays from ROIAlign's discontinuities: (sample, ratio, exact).

    ``sample``: the smallest distance of any sample coordinate from the validity cuts -1, H (y) and -1, W (x).  ``ratio``: with
    ``sampling_ratio`` 0, the smallest distance of roi_h / PH and roi_w / PW from an integer (inf otherwise).  A quantity that lies
    EXACTLY on its cut (distance 0.0; in ``also``, the same case restated in the other precision, as well when given) is left out of
    both minima and counted in ``exact``: these are the dyadic coordinates a case puts on a cut on purpose, where both precisions
    compute the same number and therefore decide alike."""
    inf = float("inf")
    sample, ratio, exact = inf, inf, 0
    others = also if also is not None else [None] * len(qs)
    for q, o in zip(qs, others):
        if q["y"].numel():
            d = torch.stack(((q["y"] + 1.0).abs(), (q["y"] - H).abs(), (q["x"] + 1.0).abs(), (q["x"] - W).abs()))
            on = d == 0
            if o is not None:
                d2 = torch.stack(((o["y"] + 1.0).abs(), (o["y"] - H).abs(), (o["x"] + 1.0).abs(), (o["x"] - W).abs())) \
                    if o["y"].shape == q["y"].shape else torch.full_like(d, inf)
                on = on & (d2 == 0)
                d = torch.minimum(d, d2)
            exact += int(on.sum())
            if (~on).any():
                sample = min(sample, float(d[~on].min()))
        if sampling_ratio <= 0:
            for key in ("ratio_h", "ratio_w"):
                d = abs(q[key] - round(q[key]))
                on = d == 0
                if o is not None:
                    d2 = abs(o[key] - round(o[key]))
                    on, d = on and d2 == 0, min(d, d2)
                if on:
                    exact += 1
                else:
                    ratio = min(ratio, d)
    return sample, ratio, exact


# ------------------------------------------------------------------------------------------------ the ROI list of the op-level tests
# Written in FEATURE coordinates of the sampling frame (image coordinate * scale - 0.5) with few mantissa bits, and converted to image
# coordinates by a power-of-two scale: the fp32 ROI the kernel reads and the float64 ROI the reference reads are the same numbers.
MAP_H, MAP_W = 40, 48


def _img(f, scale):
    return (f + 0.5) / scale


def axis_rois(scale, n_img=2, H=MAP_H, W=MAP_W):
    """-> (rois (R, 5) fp32, names).  Every class of axis-aligned ROI the tile kernel treats differently; batch indices alternate."""
    f = [
        ("tiles3x3", 5.296875, 3.640625, 40.5, 38.84375),          # ~35 x 35 px from pixel (5, 3): three 16-px tiles each way, corners on seams
        ("whole_map_margin", -3.3125, -2.703125, W + 3.21875, H + 3.109375),
        ("past_top_left", -4.203125, -3.109375, 10.40625, 12.21875),
        ("past_bottom_right", W - 11.703125, H - 9.796875, W + 7.109375, H + 7.296875),
        ("outside_right", W + 12.0, H + 10.0, W + 22.0, H + 18.0),
        ("outside_top_left", -30.0, -30.0, -10.0, -12.0),
        ("first_row_on_minus1", 7.25, -1.5, 20.609375, 12.5),      # bin_h = 2 exactly: first sample row at y = -1 (still valid)
        ("last_row_on_H", 9.125, H - 13.5, 23.484375, H + 0.5),    # last sample row at y = H (still valid)
        ("inside_one_cell", 10.3125, 12.1875, 10.59375, 12.703125),
        ("on_pixel_centre", 19.96875, 14.96875, 20.03125, 15.03125),
        ("clamp_00", -0.875, -0.875, -0.625, -0.625),
        ("clamp_0W", W - 0.75, -0.875, W - 0.25, -0.625),
        ("clamp_H0", -0.875, H - 0.75, -0.625, H - 0.25),
        ("clamp_HW", W - 0.75, H - 0.75, W - 0.25, H - 0.25),
        ("zero_extent", 12.0, 9.0, 12.0, 9.0),
        ("zero_width", 12.0, 9.0, 12.0, 20.203125),
        ("negative_extent", 20.0, 18.0, 14.109375, 10.203125),
        ("overlap_a", 8.203125, 6.296875, 22.703125, 19.40625),
        ("overlap_b", 14.109375, 10.59375, 30.296875, 27.203125),
        ("duplicate_of_overlap_a", 8.203125, 6.296875, 22.703125, 19.40625),
    ]
    rows = [[float(i % n_img)] + [_img(v, scale) for v in r[1:]] for i, r in enumerate(f)]
    return torch.tensor(rows, dtype=torch.float32), [r[0] for r in f]


def rotated_rois(scale, n_img=2, H=MAP_H, W=MAP_W):
    """-> (rois (R, 6) fp32, names): [batch, cx, cy, w, h, angle_deg]."""
    f = [("angle_%g" % a, 22.203125 + 0.5 * i, 18.609375 - 0.25 * i, 14.296875, 9.203125, a)
         for i, a in enumerate((0.0, 90.0, -90.0, 180.0, 45.0, 30.0, -75.0))]
    f += [
        ("slender_100x4_37", 23.109375, 19.296875, 25.0, 1.0, 37.0),        # 100 x 4 image px at scale 0.25
        ("slender_4x100_m53", 25.203125, 20.109375, 1.0, 25.0, -53.0),
        ("slender_long_37", 24.296875, 19.703125, 44.203125, 2.109375, 37.0),     # crosses three tiles diagonally
        ("corner_outside", 3.203125, 4.109375, 12.296875, 8.203125, 30.0),
        ("corner_outside_br", W - 3.609375, H - 2.796875, 13.109375, 7.296875, -20.0),
        ("zero_w", 20.0, 15.0, 0.0, 9.203125, 25.0),
        ("zero_h", 21.0, 16.0, 11.296875, 0.0, -40.0),
        ("sub_pixel", 30.3125, 9.1875, 0.40625, 0.296875, 60.0),
    ]
    rows = [[float(i % n_img), _img(r[1], scale), _img(r[2], scale), r[3] / scale, r[4] / scale, r[5]] for i, r in enumerate(f)]
    return torch.tensor(rows, dtype=torch.float32), [r[0] for r in f]


# ROIs that sit on a discontinuity ON PURPOSE, with dyadic numbers both precisions compute exactly (cut_distance counts them in ``exact``)
ON_A_CUT = ("first_row_on_minus1", "last_row_on_H", "zero_extent", "zero_width", "zero_w", "zero_h")


def check_cuts(rois, names, q64, q32, H, W, sampling_ratio, margin=1e-3, exact_ok=False):
    """The condition every ROIAlign comparison rests on: restated in float64 AND in fp32, no sample lies within ``margin`` px of a
    validity cut and (sampling ratio 0) no roi / P within ``margin`` of an integer, except exactly-on-the-cut quantities of the ROIs
    named in ON_A_CUT (of any ROI with ``exact_ok``).  -> (sample, ratio, exact) of the whole case."""
    for i, name in enumerate(names):
        smp, rat, exact = cut_distance(q64[i:i + 1], H, W, sampling_ratio, also=q32[i:i + 1])
        assert smp > margin and rat > margin, (name, rois[i].tolist(), smp, rat)
        assert exact == 0 or exact_ok or name in ON_A_CUT, (name, exact)
        assert (q64[i]["gh"], q64[i]["gw"]) == (q32[i]["gh"], q32[i]["gw"]), name
        assert torch.equal(q64[i]["valid"], q32[i]["valid"]), name
    return cut_distance(q64, H, W, sampling_ratio, also=q32)
