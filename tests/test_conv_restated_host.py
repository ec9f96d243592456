"""Host-side checks (no GPU) of tests/conv_restated.py, the float64 restatement tests/test_gpu_conv_elem.py holds the implicit-GEMM
convolution kernels to.  For EVERY case of every table:

* the restatement agrees with oracle/nn.py (``conv2d``, ``conv2d_backward``) - for the grouped cases with ``F.conv2d(groups=)`` and
  its autograd - to float64-vs-fp32 accuracy (the fp32 oracle is itself a sum of n fp32 addends: it is held to ``n u A``);
* an fp32 emulation of a CORRECT kernel (the same fp32 sums, one round-to-nearest where the output is bf16) satisfies every bound.

Largest |err| / bound of the emulation per table (2026-10-21): forward bf16 0.997, forward fp32 0.047, data gradient bf16 0.997,
weight gradient 0.071 (a single, mostly padded tile; 0.01 elsewhere).  No bound needed a correction.

Then twelve kinds of wrong answer are rejected (ratio > 1), and for four of them - truncating store, double rounding, bias rounded
to bf16, one dropped term among wide-range channels - the criterion of tests/test_gpu_conv.py (``max |err| <= 2^-7 max |ref|``) is
shown to ACCEPT them: the gap the per-element bounds close.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_restated as R
from oracle import nn as onn

BF16_REL = 2.0 ** -7          # tests/test_gpu_conv.py, bf16 outputs


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv32(c, bias=None):
    """fp32 convolution of a forward case (NHWC), through oracle/nn.py where it can state the case (groups == 1)."""
    if c.groups == 1:
        return onn.conv2d(c.x, c.w, bias, c.stride, c.pad, c.dil)
    return _nhwc(F.conv2d(_nchw(c.x), _nchw(c.w), bias, stride=c.stride, padding=c.pad, dilation=c.dil, groups=c.groups))


def emulate_fwd(c, form):
    """What a correct kernel stores, up to the order of its fp32 additions (fp32, BEFORE the store's rounding), and whether it is bf16."""
    if form == "plain":
        return _conv32(c), True
    if form == "bias_relu":
        return torch.relu(_conv32(c, c.bias)), True
    if form in ("bias_res_relu", "bits"):
        return torch.relu(_conv32(c, c.bias) + c.res), True
    if form == "out_f32":
        return _conv32(c, c.bias), False
    if form in ("up2", "up2_f32"):
        return onn.conv2d(c.x, c.w, c.bias, c.stride, c.pad, c.dil, res=c.res_half, res_up2=True), form == "up2"
    raise KeyError(form)


def _dgrad32(c, dy=None):
    dy = c.dy if dy is None else dy
    x0 = torch.zeros(c.N, c.H, c.W, c.C)
    if c.groups == 1:
        return onn.conv2d_backward(x0, c.w, dy, c.stride, c.pad, c.dil)[0]
    xn = _nchw(x0).requires_grad_(True)
    y = F.conv2d(xn, _nchw(c.w), None, stride=c.stride, padding=c.pad, dilation=c.dil, groups=c.groups)
    return _nhwc(torch.autograd.grad(y, xn, _nchw(dy))[0])


def emulate_dgrad(c, form):
    dx = _dgrad32(c)
    if form in ("accum", "accum_mask", "accum_bits"):
        dx = dx + c.accum
    if form == "accum_even":
        dx = dx + R.zero_stuffed(c.accum_half)
    if form in ("mask", "accum_mask", "accum_bits", "accum_even"):
        dx = dx * (c.mask > 0)
    return dx


def emulate_wgrad(c, dys=None):
    tot = 0
    for dy, x in zip(dys or c.dys, c.xs):
        if c.groups == 1:
            tot = tot + onn.conv2d_backward(x, torch.zeros(c.K, c.R, c.R, c.C), dy, c.stride, c.pad, c.dil)[1]
        else:
            wn = torch.zeros(c.K, c.C // c.groups, c.R, c.R, requires_grad=True)
            y = F.conv2d(_nchw(x), wn, None, stride=c.stride, padding=c.pad, dilation=c.dil, groups=c.groups)
            tot = tot + torch.autograd.grad(y, wn, _nchw(dy))[0].permute(0, 2, 3, 1)
    return tot


@functools.lru_cache(maxsize=None)
def _fwd(name):
    return R.fwd_inputs(name)


@functools.lru_cache(maxsize=None)
def _dg(name):
    return R.dgrad_inputs(name)


@functools.lru_cache(maxsize=None)
def _wg(name):
    return R.wgrad_inputs(name)


def _is_bf16(t):
    return bool((R.rb(t) == t).all())


# ------------------------------------------------------------------ every case: oracle agreement and the emulation within bounds
@pytest.mark.parametrize("name", list(R.FWD_CASES))
def test_forward_cases(name):
    c = _fwd(name)
    assert _is_bf16(c.x) and _is_bf16(c.w) and _is_bf16(c.res)
    out = {}
    for form in c.forms or R.FWD_ALL:
        ref, A, n, bf16 = R.fwd_reference(c, form)
        emu, _ = emulate_fwd(c, form)
        out[form + " oracle"] = R.check(emu, ref, A, n, False, name + " " + form + " vs oracle")            # float64 vs fp32
        if bf16:
            out[form + " bf16"] = R.check(R.rb(emu), ref, A, n, True, name + " " + form + " emulation")
    print("RATIO", name, {k: "%.4f" % v["ratio"] for k, v in out.items()})
    assert all(v["compared"] > 0 for v in out.values())


@pytest.mark.parametrize("name", list(R.DGRAD_CASES))
def test_data_gradient_cases(name):
    c = _dg(name)
    assert _is_bf16(c.dy) and _is_bf16(c.w) and _is_bf16(c.accum) and _is_bf16(c.mask)
    m = c.mask.view(-1)
    assert bool((m == 0).any()) and bool(torch.signbit(m[m == 0]).any()) and bool((~torch.signbit(m[m == 0])).any())     # +0.0 and -0.0
    out = {}
    for form in c.forms or R.DG_ALL:
        ref, A, n = R.dgrad_reference(c, form)
        emu = emulate_dgrad(c, form)
        out[form + " oracle"] = R.check(emu, ref, A, n, False, name + " " + form + " vs oracle")
        out[form + " bf16"] = R.check(R.rb(emu), ref, A, n, True, name + " " + form + " emulation")
    print("RATIO", name, {k: "%.4f" % v["ratio"] for k, v in out.items()})


@pytest.mark.parametrize("name", list(R.WGRAD_CASES))
def test_weight_gradient_cases(name):
    c = _wg(name)
    emu = emulate_wgrad(c)
    out = {"plain": R.check(emu, *R.wgrad_reference(c), False, name + " dW")}
    out["x2"] = R.check((emu + emu) / 2, *R.wgrad_reference(c), False, name + " dW accumulated")
    assert bool((torch.frexp(c.qscale)[0] == 0.5).all())                                                   # exact powers of two
    out["qscale"] = R.check(emu * c.qscale.view(-1, 1, 1, 1), *R.wgrad_reference(c, qscale=True), False, name + " dW qscale")
    print("RATIO", name, {k: "%.4f" % v["ratio"] for k, v in out.items()})


def test_multilevel_and_split_shapes():
    """The multi-level (64 -> 128) and split-dispatch (256 -> 256) cases of the device test are forward / data-gradient cases per level."""
    for levels, C, K in ((R.ML_LEVELS, 64, 128), (R.SPLIT_LEVELS, 256, 256)):
        for i, hw in enumerate(levels):
            tab = {"lvl%d" % i: R._f((2,) + hw, C, K)}
            c = R.fwd_inputs("lvl%d" % i, tab)
            for form in ("bias_relu", "out_f32"):
                ref, A, n, bf16 = R.fwd_reference(c, form)
                emu, _ = emulate_fwd(c, form)
                R.check(R.rb(emu) if bf16 else emu, ref, A, n, bf16, "level %s %s" % (hw, form))
            tab = {"lvl%d" % i: R._d((2,) + hw, C, K)}
            d = R.dgrad_inputs("lvl%d" % i, tab)
            ref, A, n = R.dgrad_reference(d, "accum_mask")
            R.check(R.rb(emulate_dgrad(d, "accum_mask")), ref, A, n, True, "level %s dgrad" % (hw,))


def test_dispatch_plan_names_the_cases_kernels():
    """sod_conv_plan walks dispatch_conv without launching: every single-level forward / data-gradient case reaches the kernel variant
    it names (for a 256-CU device, the plan's default), so a table entry cannot drift off its path unnoticed on a machine without a GPU."""
    import ctypes

    from slenderobjdet_amd import _C

    lib = _C.load()
    for mode, table in ((0, R.FWD_CASES), (1, R.DGRAD_CASES)):
        for name, c in table.items():
            if c["groups"] > 1:
                continue                                # the channel window has its own entry points
            N, H, W = c["shape"]
            try:
                for k, v in c["knobs"].items():
                    assert getattr(lib, k)(v) == 0
                v = lib.sod_conv_plan(mode, 1, N, (ctypes.c_int * 1)(H), (ctypes.c_int * 1)(W), c["C"], c["K"], c["R"], c["R"], c["stride"], c["pad"],
                                      c["dil"], None, None)
            finally:
                for k in c["knobs"]:
                    getattr(lib, k)(0 if k == "sod_conv_set_reverse" else -1)
            assert v == c["variant"], (mode, name, v, c["variant"])


# ------------------------------------------------------------------ wrong answers
def _truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _rejected(got, ref, A, n, bf16, what, accepted_by_current=None):
    r = R.check(got, ref, A, n, bf16, what, enforce=False)
    cur = R.current_criterion(got, ref, BF16_REL)
    print("WRONG %-44s ratio %8.3g  over %5.1f %%  current criterion %.2f" % (what, r["ratio"], 100 * R.over(got, ref, A, n, bf16), cur))
    assert r["ratio"] > 1.0, (what, r)
    if accepted_by_current:
        assert cur <= 1.0, (what, "the current criterion was expected to accept this", cur)
    return r


def test_truncating_store_is_rejected():
    c = _fwd("l128_3x3_iid")
    ref, A, n, _ = R.fwd_reference(c, "plain")
    _rejected(_truncate_bf16(emulate_fwd(c, "plain")[0]), ref, A, n, True, "fwd truncating store", True)
    d = _dg("l128_3x3_iid")
    ref, A, n = R.dgrad_reference(d, "plain")
    _rejected(_truncate_bf16(emulate_dgrad(d, "plain")), ref, A, n, True, "dgrad truncating store", True)


def test_double_rounding_is_rejected():
    c = _fwd("l128_3x3_iid")
    kw = dict(groups=1, **c.geo)
    ref, A, n = R.forward(c.x, c.w, c.bias, **kw)
    _rejected(R.rb(R.rb(_conv32(c)) + c.bias), ref, A, n, True, "fwd round, add bias, round", True)
    ref, A, n = R.forward(c.x, c.w, None, c.res, **kw)
    _rejected(R.rb(R.rb(_conv32(c)) + c.res), ref, A, n, True, "fwd round, add residual, round", True)
    d = _dg("l128_3x3_iid")
    ref, A, n = R.dgrad_reference(d, "accum")
    _rejected(R.rb(R.rb(_dgrad32(d)) + d.accum), ref, A, n, True, "dgrad round, add accum, round", True)


def test_bias_rounded_to_bf16_is_rejected():
    c = _fwd("l128_3x3_iid")
    ref, A, n = R.forward(c.x, c.w, c.bias, **c.geo)
    _rejected(R.rb(_conv32(c) + R.rb(c.bias)), ref, A, n, True, "fwd bias rounded to bf16", True)


def test_dropped_contraction_term_is_rejected():
    """One (tap, channel) term of every dx element is missing; the channel is one of the SMALL ones of the wide-range dY (2^-3)."""
    d = _dg("l128_3x3")
    k0 = 7                                                           # 7 % 7 == 0: scale 2^-3
    assert float(R.red_scale(d.K)[k0]) == 2.0 ** -3
    dy1, w1 = torch.zeros_like(d.dy), torch.zeros_like(d.w)
    dy1[..., k0] = d.dy[..., k0]
    w1[k0, 1, 1] = d.w[k0, 1, 1]
    term = R.dgrad(dy1, w1, (d.H, d.W), **d.geo)[0]
    assert float(term.abs().max()) > 0
    ref, A, n = R.dgrad_reference(d, "plain")
    _rejected(R.rb(_dgrad32(d) - term.float()), ref, A, n, True, "dgrad one term dropped (2^-3 channel)", True)
    c = _fwd("l128_3x3")
    x1, w1 = torch.zeros_like(c.x), torch.zeros_like(c.w)
    x1[..., 7] = c.x[..., 7]
    w1[:, 1, 1, 7] = c.w[:, 1, 1, 7]
    ref, A, n, _ = R.fwd_reference(c, "plain")
    _rejected(R.rb(_conv32(c) - R.forward(x1, w1, **c.geo)[0].float()), ref, A, n, True, "fwd one term dropped (2^-3 channel)")


def test_dropped_tap_at_a_corner_pixel_is_rejected():
    c = _fwd("l128_3x3")
    ref, A, n, _ = R.fwd_reference(c, "plain")
    y = _conv32(c)
    y[0, 0, 0] -= c.w[:, 1, 1] @ c.x[0, 0, 0]
    _rejected(R.rb(y), ref, A, n, True, "fwd centre tap dropped at pixel (0, 0)")
    y = _conv32(c)
    y[-1, -1, -1] -= c.w[:, 0, 0] @ c.x[-1, -2, -2]
    _rejected(R.rb(y), ref, A, n, True, "fwd tap (0, 0) dropped at the last pixel")


def test_bias_missing_from_the_last_channels_is_rejected():
    c = _fwd("l128_p128_k136")
    ref, A, n, _ = R.fwd_reference(c, "bias_relu")
    b = c.bias.clone()
    b[-8:] = 0
    _rejected(R.rb(torch.relu(_conv32(c, b))), ref, A, n, True, "fwd bias missing from the last 8 channels")
    ref, A, n, _ = R.fwd_reference(c, "out_f32")
    _rejected(_conv32(c, b), ref, A, n, False, "fwd (fp32) bias missing from the last 8 channels")


def test_swapped_small_channels_are_rejected():
    c = _fwd("l128_3x3")
    k0 = 13                                                          # 13 % 13 == 0: the smallest scale, 2^-6; 13 and 14 share a lane's 8
    assert float(R.out_scale(c.K)[k0]) == 2.0 ** -6 and k0 // 8 == (k0 + 1) // 8
    ref, A, n, _ = R.fwd_reference(c, "plain")
    y = R.rb(_conv32(c))
    y[..., [k0, k0 + 1]] = y[..., [k0 + 1, k0]]
    r = _rejected(y, ref, A, n, True, "fwd channels 13 / 14 swapped")
    assert R.current_criterion(y, ref, BF16_REL) <= 1.0              # invisible in the max norm: these channels are 2^-12 of the largest
    d = _dg("l128_3x3")
    ref, A, n = R.dgrad_reference(d, "plain")
    dx = R.rb(_dgrad32(d))
    dx[..., [k0, k0 + 1]] = dx[..., [k0 + 1, k0]]
    _rejected(dx, ref, A, n, True, "dgrad channels 13 / 14 swapped", True)
    assert r["ratio"] > 100


def test_mask_ge_zero_is_rejected():
    d = _dg("l128_3x3")
    for form in ("mask", "accum_mask"):
        ref, A, n = R.dgrad_reference(d, form)
        dx = _dgrad32(d) + (d.accum if form == "accum_mask" else 0)
        r = _rejected(R.rb(dx * (d.mask >= 0)), ref, A, n, True, "dgrad %s: mask >= 0" % form)
        assert r["ratio"] > 1e100                                    # a zero bound: masked elements must be exactly zero
        neg0 = torch.signbit(d.mask) & (d.mask == 0)
        wrong = torch.where(neg0, torch.zeros_like(dx), dx * (d.mask >= 0))         # right at -0.0, wrong at +0.0 only
        _rejected(R.rb(wrong), ref, A, n, True, "dgrad %s: mask >= 0 except at -0.0" % form)


def test_accum_even_added_at_odd_pixels_is_rejected():
    for name in ("even_1x1", "even_3x3"):
        d = _dg(name)
        ref, A, n = R.dgrad_reference(d, "accum_even")
        ok = emulate_dgrad(d, "accum_even")
        R.check(R.rb(ok), ref, A, n, True, name)
        wrong = (_dgrad32(d) + R.up2(d.accum_half)) * (d.mask > 0)
        _rejected(R.rb(wrong), ref, A, n, True, name + ": residual at odd pixels too")
        # every parity of (h, w) and the last row / column are part of the comparison: a wrong value there alone is seen
        for h, w in ((0, 1), (1, 0), (1, 1), (d.H - 1, d.W - 1), (d.H - 2, d.W - 2)):
            one = R.rb(ok.clone())
            keep = d.mask[0, h, w] > 0
            one[0, h, w] = torch.where(keep, wrong[0, h, w] + R.rb(ok)[0, h, w] + 1.0, one[0, h, w])
            assert R.check(one, ref, A, n, True, enforce=False)["ratio"] > 1.0, (name, h, w)


def test_up2_residual_with_the_full_width_is_rejected():
    c = _fwd("up2_1x1")
    ref, A, n, _ = R.fwd_reference(c, "up2")
    ph, pw = torch.meshgrid(torch.arange(c.Ho), torch.arange(c.Wo), indexing="ij")
    rows = c.res_half.reshape(c.N, -1, c.K)
    idx = ((ph // 2) * c.Wo + pw // 2).reshape(-1).clamp_max(rows.shape[1] - 1)                  # Wp instead of Wp / 2
    wrong = _conv32(c, c.bias) + rows[:, idx].reshape(c.N, c.Ho, c.Wo, c.K)
    _rejected(R.rb(wrong), ref, A, n, True, "fwd up-sampled residual indexed with Wp")
    _rejected(wrong, *R.fwd_reference(c, "up2_f32")[:3], False, "fwd (fp32) up-sampled residual indexed with Wp")


def test_weight_gradient_wrong_answers_are_rejected():
    for name in ("w128_wide_row", "w9_k136", "w256_k264_1x1", "fold_k8"):
        c = _wg(name)
        dys = [d.clone() for d in c.dys]
        dys[-1][-1, -1, -1] = 0
        _rejected(emulate_wgrad(c, dys), *R.wgrad_reference(c), False, name + ": dW without the last pixel of the last image")
        emu = emulate_wgrad(c)
        _rejected(emu * torch.roll(c.qscale, 1).view(-1, 1, 1, 1), *R.wgrad_reference(c, qscale=True), False, name + ": qscale of the neighbouring channel")


def test_half_ulp_and_measure():
    v = torch.tensor([0.0, 1.0, 1.5, 1.9999, 2.0, 0.75, 3.0e-5], dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -24], dtype=torch.float64)
    assert torch.equal(R.half_ulp_bf16(v), want)
    # a value exactly half way between two bf16 numbers is within the bound, one fp32 ulp further is not
    ref = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)
    zero = torch.zeros(1, dtype=torch.float64)
    assert R.check(torch.tensor([1.0]), ref, zero, 1, True, enforce=False)["ratio"] == 1.0
    assert R.check(torch.tensor([1.0 - 2.0 ** -8]), ref, zero, 1, True, enforce=False)["ratio"] > 1.0
    r = R.check(torch.tensor([float("nan")]), ref, zero, 1, True, enforce=False)
    assert not r["same_nonfinite"]
    r = R.check(torch.tensor([1.0]), torch.tensor([float("nan")], dtype=torch.float64), zero, 1, True, enforce=False)
    assert not r["same_nonfinite"]
    assert R.check(torch.tensor([1e-30]), zero, zero, 1, True, enforce=False)["ratio"] > 1.0          # zero bound: exact or rejected
    b = torch.rand(4, 16) > 0.5
    assert torch.equal(R.bits_unpack(R.bits_pack(b), b.shape), b)
