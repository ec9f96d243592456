"""The implicit-GEMM convolution kernels (csrc/conv_igemm.hip, conv_igemm256.hip, conv_pw.hip, conv_ws3.hip, the weight-gradient
kernels, chosen by conv_dispatch.hip) against the float64 restatement of tests/conv_restated.py, PER ELEMENT and with no element left
out.  Every bound is the restatement's (derived there from the number formats, the number of addends and the absolute-addend sums;
nothing is tuned to what the kernels give).  tests/test_conv_restated_host.py shows on the CPU that the same checks pass a correct
fp32 / bf16 emulation and reject twelve kinds of wrong answer, for the cases used here.

Every case names the kernel it is about and FAILS when the dispatch goes elsewhere: ``sod_conv_last_variant()`` /
``sod_conv_last_tail_variant()`` for forward and data gradient, the ``variant`` column of ``sod_conv_prof_collect`` for the weight
gradients (32003 conv_wgrad_kernel, 2300 / 2310 conv_wgrad_ring.hip, 256 conv_wgrad256, 9009 conv_wgrad9, 32004 conv_wgrad_fold).
Outputs sit between 4 KB of sentinel bytes that must survive; inputs sit between NaNs, so that an out-of-range read that enters a sum
shows as a non-finite element.

Which case reaches which kernel follows dispatch_conv (conv_dispatch.hip): Nout <= 16 -> 16x256, Nout <= 64 -> 64x256 (BK = 32 when
the channels allow), else 128x128 with BK = 32 above 512 workgroups (TILE_128x128_K32: (1, 65, 127) x 1024 output channels = 520
workgroups; P = 8255 < 16384 keeps the 128-channel 1x1 case off conv_pw); a channel count that is no multiple of 64 takes the gather
form (code + 1).  The data gradient of a convolution C -> K stores C channels, so the issue's "dgrad of (2, 15, 13) 64 -> 128 at
stride 2" is a 64x256 tile (kept, as t64_s2_odd); the 128x128 data-gradient cases have 128 input channels.

Worst |err| / bound per path, measured on one MI355X against the float64 reference on 2026-10-21 (bf16 output / fp32 output; the
RATIO lines of a run give every figure; these are measurements, no bound is derived from them):

    forward        12812864 0.996 / 0.016   12812865 0.930 / 0.002   12812832 0.997 / 0.024   6425632 0.922 / 0.002   6425665 0.957 / 0.003
                   1625664 0.917 / 0.001    1625665 0.881 / 0.001    256 0.992 / 0.012        7003 0.885              7001 0.995
                   channel window 0.996     split remainder 0.753    multi-level 0.943 / 0.002
    data gradient  12812864 0.971           12812865 0.941           12812832 0.997           6425632 0.990 (accum_even)  1625664 0.784
                   256 0.944                7003 0.886               7001 0.994               channel window 0.997    k_pitch 0.941
                   split remainder 0.698    multi-level 0.875
    weight grad.   32003 0.007   ring 2300 / 2310 0.007   256 0.056   9009 0.048   32004 0.002   diagonal tiles 0.004   deterministic 0.005

No case needed a kernel fix.  One finding about the existing suite: with ``splits=0`` the 3x3 shapes with 64 or 72 output channels go to
conv_wgrad_fold BEFORE sod_conv_set_wgrad_variant is looked at, so test_conv_wgrad_ring_variants never ran the ring kernel on them; here
they reach it through an explicit split count (_fold_takes).
"""
import contextlib
import ctypes
import functools

import pytest
import torch

import conv_restated as R

pytestmark = pytest.mark.gpu

# name of the knob -> the value that hands it back to the environment / default
_RESTORE = {"sod_conv_set_reverse": 0}
T128, T64x128, T64x64, T64x64_R3 = 12812864, 6412864, 6406464, 36406464
W128, WFOLD, W256, W9 = 32003, 32004, 256, 9009


@contextlib.contextmanager
def _knobs(knobs):
    from slenderobjdet_amd import _C

    try:
        for k, v in knobs.items():
            _C.call(k, v)
        yield
    finally:
        for k in knobs:
            _C.call(k, _RESTORE.get(k, -1))


def _variant():
    from slenderobjdet_amd import _C

    return int(_C.load().sod_conv_last_variant())


def _tail_variant():
    from slenderobjdet_amd import _C

    return int(_C.load().sod_conv_last_tail_variant())


def _show(name, out):
    print("RATIO", name, {k: "%.3f" % v["ratio"] for k, v in out.items()})


def _assert_all(name, out):
    _show(name, out)
    for k, v in out.items():
        assert v["same_nonfinite"], (name, k, "the non-finite elements are not the reference's")
        assert v["ratio"] <= 1.0 and v["compared"] > 0, (name, k, v)


@functools.lru_cache(maxsize=None)
def _fwd_case(name):
    return R.fwd_inputs(name)


@functools.lru_cache(maxsize=None)
def _fwd_ref(name, form):
    c = _fwd_case(name)
    if form == "pre":                                   # bias + residual, before the ReLU: what the 1-bit mask decides on
        return R.forward(c.x, c.w, c.bias, c.res, groups=c.groups, **c.geo) + (True,)
    if form == "bits":
        form = "bias_res_relu"
    return R.fwd_reference(c, form)


@functools.lru_cache(maxsize=None)
def _dg_case(name):
    return R.dgrad_inputs(name)


@functools.lru_cache(maxsize=None)
def _dg_ref(name, form):
    return R.dgrad_reference(_dg_case(name), "accum_mask" if form == "accum_bits" else form)


@functools.lru_cache(maxsize=None)
def _wg_case(name):
    return R.wgrad_inputs(name)


@functools.lru_cache(maxsize=None)
def _wg_ref(name, qscale):
    return R.wgrad_reference(_wg_case(name), qscale=qscale)


def _grouped(c, cuda):
    """The channel-window weights of a grouped case: forward (K, R, S, 128) and transposed, as layers/nn.py builds them."""
    from slenderobjdet_amd.layers.nn import HipGroupedConv2d

    m = HipGroupedConv2d(c.C, c.K, c.R, c.stride, c.pad, c.dil, groups=c.groups, bias=False).to(cuda)
    assert m.windowed()
    win = m.window_weight(c.w.to(cuda))
    T = c.C // 128
    win_t = win.reshape(T, 128, c.R, c.R, 128).permute(0, 4, 2, 3, 1).reshape(win.shape)
    return m, win.contiguous().bfloat16(), win_t.contiguous().bfloat16()


# ------------------------------------------------------------------ forward
def _fwd_args(form):
    """(bias?, residual: None / "full" / "half", relu, out_f32, bits)"""
    return {"plain": (False, None, False, False, False), "bias_relu": (True, None, True, False, False),
            "bias_res_relu": (True, "full", True, False, False), "out_f32": (True, None, False, True, False),
            "up2": (True, "half", False, False, False), "up2_f32": (True, "half", False, True, False),
            "bits": (True, "full", True, False, True)}[form]


@pytest.mark.parametrize("name", list(R.FWD_CASES))
def test_forward_per_element(cuda, name):
    from slenderobjdet_amd.layers import functional as HF

    c = _fwd_case(name)
    x = R.in_nan_arena(c.x, cuda)
    w = _grouped(c, cuda)[1] if c.groups > 1 else R.in_nan_arena(c.w, cuda)
    bias = c.bias.to(cuda)
    res = {"full": R.in_nan_arena(c.res, cuda), "half": None if c.res_half is None else R.in_nan_arena(c.res_half, cuda)}
    out = {}
    with _knobs(c.knobs):
        for form in c.forms or R.FWD_ALL:
            has_bias, which, relu, out_f32, with_bits = _fwd_args(form)
            y, guard = R.guarded((c.N, c.Ho, c.Wo, c.K), torch.float32 if out_f32 else torch.bfloat16, cuda)
            bits, bguard = R.guarded((y.numel() // 8,), torch.uint8, cuda) if with_bits else (None, None)
            got = HF.conv2d_fwd(x, w, bias if has_bias else None, res[which] if which else None, stride=c.stride, pad=c.pad, dil=c.dil, relu=relu,
                                res_up2=which == "half", out_f32=out_f32, out=y, relu_bits=bits)
            assert _variant() == c.variant, (name, form, "ran on variant %d, the case is about %d" % (_variant(), c.variant))
            torch.cuda.synchronize()
            assert got.data_ptr() == y.data_ptr()
            R.assert_guards_intact(guard, name + " " + form)
            ref, A, n, bf16 = _fwd_ref(name, form)
            assert bf16 == (not out_f32)
            yc = y.float().cpu()
            out[form] = R.check(yc, ref, A, n, bf16, enforce=False)
            if with_bits:
                R.assert_guards_intact(bguard, name + " relu bits")
                stored = R.bits_unpack(bits.cpu(), yc.shape)
                assert torch.equal(stored, yc > 0), (name, "the bits are not (stored y > 0)")
                pre, pA, pn, _ = _fwd_ref(name, "pre")
                decided = pre.abs() > R.bound_bf16(pre, pA, pn)           # per element: outside its own bound the sign is the reference's
                assert torch.equal(stored[decided], (pre > 0)[decided]), (name, "a bit differs where the pre-activation is decided")
                assert 0.2 < float(stored.float().mean()) < 0.8 and float(decided.float().mean()) > 0.5
    _assert_all("fwd " + name, out)


# ------------------------------------------------------------------ data gradient
def _run_dgrad(HF, cuda, c, form, dy, wt, ops):
    dx, guard = R.guarded((c.N, c.H, c.W, c.C), torch.bfloat16, cuda)
    kw = {}
    if form in ("accum", "accum_mask", "accum_bits"):
        kw["accum"] = ops["accum"]
    if form in ("mask", "accum_mask"):
        kw["relu_mask"] = ops["mask"]
    if form in ("accum_bits", "accum_even"):
        kw["relu_bits"] = ops["bits"]
    if form == "accum_even":
        kw.update(accum=ops["accum_half"], accum_even=True)
    got = HF.conv2d_dgrad(dy, wt, (c.H, c.W), c.stride, c.pad, c.dil, out=dx, **kw)
    v = _variant()
    torch.cuda.synchronize()
    assert got.data_ptr() == dx.data_ptr()
    R.assert_guards_intact(guard, "dgrad " + form)
    return dx.float().cpu(), v


@pytest.mark.parametrize("name", list(R.DGRAD_CASES))
def test_data_gradient_per_element(cuda, name):
    from slenderobjdet_amd.layers import functional as HF

    c = _dg_case(name)
    dy = R.in_nan_arena(c.dy, cuda)
    wt = _grouped(c, cuda)[2] if c.groups > 1 else R.in_nan_arena(c.w.permute(3, 1, 2, 0).contiguous(), cuda)
    ops = {"accum": R.in_nan_arena(c.accum, cuda), "mask": R.in_nan_arena(c.mask, cuda), "bits": R.bits_pack(c.mask > 0).to(cuda),
           "accum_half": None if c.accum_half is None else R.in_nan_arena(c.accum_half, cuda)}
    out = {}
    with _knobs(c.knobs):
        for form in c.forms or R.DG_ALL:
            dx, v = _run_dgrad(HF, cuda, c, form, dy, wt, ops)
            assert v == c.variant, (name, form, "ran on variant %d, the case is about %d" % (v, c.variant))
            ref, A, n = _dg_ref(name, form)
            out[form] = R.check(dx, ref, A, n, True, enforce=False)
            if form == "accum_even":                    # every parity of (h, w), the last row and the last column, each on its own
                for tag, sl in (("ee", (slice(0, None, 2), slice(0, None, 2))), ("eo", (slice(0, None, 2), slice(1, None, 2))),
                                ("oe", (slice(1, None, 2), slice(0, None, 2))), ("oo", (slice(1, None, 2), slice(1, None, 2))),
                                ("last row", (slice(c.H - 1, c.H), slice(None))), ("last col", (slice(None), slice(c.W - 1, c.W)))):
                    i = (slice(None),) + sl
                    out["even " + tag] = R.check(dx[i], ref[i], A[i], n, True, enforce=False)
                    assert float(ref[i].abs().max()) > 0
    _assert_all("dgrad " + name, out)


# ------------------------------------------------------------------ split dispatch: 256x256 main launch + remainder tile
@functools.lru_cache(maxsize=None)
def _levels_case(levels, C, K, tag):
    """Levels that share one weight: forward inputs per level, data-gradient inputs per level (dx of C channels from dY of K)."""
    f = [R.fwd_inputs("%s%d" % (tag, i), {"%s%d" % (tag, i): R._f((2,) + hw, C, K)}) for i, hw in enumerate(levels)]
    d = [R.dgrad_inputs("%s%d" % (tag, i), {"%s%d" % (tag, i): R._d((2,) + hw, C, K)}) for i, hw in enumerate(levels)]
    return f, d


@functools.lru_cache(maxsize=None)
def _levels_ref(levels, C, K, tag, what):
    f, d = _levels_case(levels, C, K, tag)
    if what == "fwd_bias_relu":
        return [R.forward(c.x, f[0].w, f[0].bias, relu=True, **c.geo) for c in f]
    if what == "fwd_f32":
        return [R.forward(c.x, f[0].w, **c.geo) for c in f]
    kw = {"dgrad": lambda c: {}, "dgrad_mask": lambda c: dict(mask=c.mask), "dgrad_accum": lambda c: dict(accum=c.accum),
          "dgrad_accum_mask": lambda c: dict(accum=c.accum, mask=c.mask)}[what]
    return [R.dgrad(c.dy, d[0].w, (c.H, c.W), **c.geo, **kw(c)) for c in d]


@pytest.mark.parametrize("tile", [0, T64x64, T64x128, T64x64_R3])
def test_split_dispatch_remainder_per_element(cuda, tile):
    """256 -> 256 3x3, N = 2, levels 16x24 + 5x7, split after two 256-pixel tiles: the remainder (the last tile of level 0 and all of
    level 1) on each of the four remainder tiles; forward bias + ReLU, data gradient accumulate + mask."""
    from slenderobjdet_amd.layers import functional as HF

    key = (tuple(R.SPLIT_LEVELS), 256, 256, "split")
    f, d = _levels_case(*key)
    xs = [R.in_nan_arena(c.x, cuda) for c in f]
    w, bias = R.in_nan_arena(f[0].w, cuda), f[0].bias.to(cuda)
    dys = [R.in_nan_arena(c.dy, cuda) for c in d]
    wt = R.in_nan_arena(d[0].w.permute(3, 1, 2, 0).contiguous(), cuda)
    masks, accs = [c.mask.to(cuda).bfloat16() for c in d], [c.accum.to(cuda).bfloat16() for c in d]
    outs = [R.guarded((2,) + hw + (256,), torch.bfloat16, cuda) for hw in R.SPLIT_LEVELS]
    with _knobs({"sod_conv_set_tail_split": 2, "sod_conv_set_tail_tile": tile}):
        HF.conv2d_fwd_ml(xs, w, bias, 1, 1, 1, relu=True, outs=[o for o, _ in outs])
        vf = (_variant(), _tail_variant())
        dxs = HF.conv2d_dgrad_ml(dys, wt, R.SPLIT_LEVELS, 1, 1, 1, relu_masks=masks, accums=accs)
        vd = (_variant(), _tail_variant())
        torch.cuda.synchronize()
    assert vf == (256, tile or T128) and vd == (256, tile or T128), (vf, vd)
    out = {}
    for l, ((y, guard), dx) in enumerate(zip(outs, dxs)):
        R.assert_guards_intact(guard, "split forward level %d" % l)
        out["fwd l%d" % l] = R.check(y.float().cpu(), *_levels_ref(*key, "fwd_bias_relu")[l], True, enforce=False)
        out["dgrad l%d" % l] = R.check(dx.float().cpu(), *_levels_ref(*key, "dgrad_accum_mask")[l], True, enforce=False)
    _assert_all("split tail %d" % tile, out)


# ------------------------------------------------------------------ multi-level launches
def test_multilevel_per_element(cuda):
    """Five levels (20, 28) ... (2, 2), 64 -> 128: conv2d_fwd_ml (bf16 with bias + ReLU; fp32 into the concatenated (N, L, K) buffer),
    conv2d_dgrad_ml plain, with relu_masks, accums, both, and from strided dY views of the concatenated buffer."""
    from slenderobjdet_amd.layers import functional as HF

    key = (tuple(R.ML_LEVELS), 64, 128, "ml")
    f, d = _levels_case(*key)
    N, C, K, hw = 2, 64, 128, R.ML_LEVELS
    xs = [R.in_nan_arena(c.x, cuda) for c in f]
    w, bias = R.in_nan_arena(f[0].w, cuda), f[0].bias.to(cuda)
    out = {}
    outs = [R.guarded((N,) + s + (K,), torch.bfloat16, cuda) for s in hw]
    HF.conv2d_fwd_ml(xs, w, bias, 1, 1, 1, relu=True, outs=[o for o, _ in outs])
    assert _variant() == R.L128
    L = sum(h * ww for h, ww in hw)
    offs = [sum(h * ww for h, ww in hw[:i]) for i in range(len(hw))]
    buf, bguard = R.guarded((N, L, K), torch.float32, cuda)
    HF.conv2d_fwd_ml(xs, w, None, 1, 1, 1, out_f32=True, outs=[buf.view(-1)[o * K:] for o in offs], y_img_stride=L * K)
    assert _variant() == R.L128
    torch.cuda.synchronize()
    R.assert_guards_intact(bguard, "concatenated fp32 output")
    for l, (y, guard) in enumerate(outs):
        R.assert_guards_intact(guard, "ml forward level %d" % l)
        out["fwd l%d" % l] = R.check(y.float().cpu(), *_levels_ref(*key, "fwd_bias_relu")[l], True, enforce=False)
        ref, A, n = _levels_ref(*key, "fwd_f32")[l]
        got = buf[:, offs[l]:offs[l] + hw[l][0] * hw[l][1]].reshape(ref.shape).cpu()
        out["concat f32 l%d" % l] = R.check(got, ref, A, n, False, enforce=False)
    # data gradient: dx of 64 channels from dY of 128 -> the 64x256 BK = 32 tile
    dys = [R.in_nan_arena(c.dy, cuda) for c in d]
    wt = R.in_nan_arena(d[0].w.permute(3, 1, 2, 0).contiguous(), cuda)
    masks, accs = [c.mask.to(cuda).bfloat16() for c in d], [c.accum.to(cuda).bfloat16() for c in d]
    gbuf = R.in_nan_arena(torch.cat([c.dy.reshape(N, -1, K) for c in d], 1), cuda)
    gviews = [gbuf.view(-1)[o * K:] for o in offs]
    runs = {"dgrad": {}, "dgrad_mask": dict(relu_masks=masks), "dgrad_accum": dict(accums=accs), "dgrad_accum_mask": dict(relu_masks=masks, accums=accs)}
    for what, kw in runs.items():
        dxs = HF.conv2d_dgrad_ml(dys, wt, hw, 1, 1, 1, **kw)
        assert _variant() == R.T64K32, (what, _variant())
        for l, dx in enumerate(dxs):
            out["%s l%d" % (what, l)] = R.check(dx.float().cpu(), *_levels_ref(*key, what)[l], True, enforce=False)
    dxs = HF.conv2d_dgrad_ml(gviews, wt, hw, 1, 1, 1, dy_img_stride=L * K, N=N)
    assert _variant() == R.T64K32
    for l, dx in enumerate(dxs):
        out["dgrad views l%d" % l] = R.check(dx.float().cpu(), *_levels_ref(*key, "dgrad")[l], True, enforce=False)
    _assert_all("multi-level", out)


@functools.lru_cache(maxsize=None)
def _kpitch_case():
    f, d = _levels_case(tuple(R.ML_LEVELS), 256, 72, "kp")
    return d, [R.dgrad(c.dy, d[0].w, (c.H, c.W), **c.geo) for c in d]


@pytest.mark.parametrize("tile256", [0, 2])
def test_multilevel_padded_contraction_per_element(cuda, tile256):
    """dY rows of 72 channels in the concatenated (N, L, 72) buffer: the per-chunk gather (12812865) of the plain entry point, and
    ``k_pitch`` - contracted as 128 channels per tap against zero-padded weights on the linear 128x128 kernel and on the 256x256 one."""
    from slenderobjdet_amd.layers import functional as HF

    d, refs = _kpitch_case()
    N, C, K, hw = 2, 256, 72, R.ML_LEVELS
    L = sum(h * ww for h, ww in hw)
    offs = [sum(h * ww for h, ww in hw[:i]) for i in range(len(hw))]
    gbuf = R.in_nan_arena(torch.cat([c.dy.reshape(N, -1, K) for c in d], 1), cuda)
    gviews = [gbuf.view(-1)[o * K:] for o in offs]
    wt = d[0].w.permute(3, 1, 2, 0).contiguous()
    wt_pad = torch.nn.functional.pad(wt, (0, 128 - K))
    out = {}
    with _knobs({"sod_conv_set_tile256": tile256}):
        plain = HF.conv2d_dgrad_ml(gviews, R.in_nan_arena(wt, cuda), hw, 1, 1, 1, dy_img_stride=L * K, N=N)
        assert _variant() == R.G128, _variant()
        got = HF.conv2d_dgrad_ml(gviews, R.in_nan_arena(wt_pad, cuda), hw, 1, 1, 1, dy_img_stride=L * K, N=N, k_pitch=K)
        assert _variant() == (R.V256 if tile256 else R.L128), _variant()
        torch.cuda.synchronize()
    for l, (p, g) in enumerate(zip(plain, got)):
        out["gather l%d" % l] = R.check(p.float().cpu(), *refs[l], True, enforce=False)
        out["k_pitch l%d" % l] = R.check(g.float().cpu(), *refs[l], True, enforce=False)
    _assert_all("padded contraction tile256=%d" % tile256, out)


# ------------------------------------------------------------------ weight gradients
def _wgrad_variants(fn):
    """Runs ``fn`` with the in-library profile on -> the kernel variant of every weight-gradient dispatch it made."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    ms, var, frac, mode = (ctypes.c_float * 64)(), (ctypes.c_int * 64)(), (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    _C.load().sod_conv_prof_collect(ms, var, frac, mode, 64)       # rows an earlier user of the profile left behind
    _C.call("sod_conv_prof_enable", 1)
    try:
        fn()
        HF.wgrad_join()
        torch.cuda.synchronize()
    finally:
        _C.call("sod_conv_prof_enable", 0)
    n =_C.load().sod_conv_prof_collect(ms, var, frac, mode, 64)
    return [int(var[i]) for i in range(n) if mode[i] == 2]


class _WDev:
    """A weight-gradient case on the device: operands between NaNs, dY also as views of the concatenated (N, L, K) buffer."""

    def __init__(self, c, cuda):
        self.c, self.cuda = c, cuda
        self.xs = [R.in_nan_arena(x, cuda) for x in c.xs]
        self.dys = [R.in_nan_arena(dy, cuda) for dy in c.dys]
        self.qs = c.qscale.to(cuda)
        P = [dy.shape[1] * dy.shape[2] for dy in c.dys]
        self.L = sum(P)
        self.gbuf = R.in_nan_arena(torch.cat([dy.reshape(c.N, -1, c.K) for dy in c.dys], 1), cuda)
        self.gviews = [self.gbuf.view(-1)[sum(P[:i]) * c.K:] for i in range(len(P))]
        self.shape = (c.K, c.R, c.R, 128 if c.kernel == "diag" else c.C)
        self.module = None
        if c.kernel == "diag":
            from slenderobjdet_amd.layers.nn import HipGroupedConv2d

            self.module = HipGroupedConv2d(c.C, c.K, c.R, c.stride, c.pad, c.dil, groups=c.groups, bias=False)

    def launch(self, dw, splits, qscale=False):
        from slenderobjdet_amd.layers import functional as HF

        c, qs = self.c, self.qs if qscale else None
        if c.kernel == "fold":
            HF.conv2d_wgrad_ml(self.gviews, self.xs, dw, c.R, c.R, c.stride, c.pad, c.dil, dy_img_stride=self.L * c.K, K=c.K, splits=splits, qscale=qs)
        elif len(self.xs) > 1:
            HF.conv2d_wgrad_ml(self.dys, self.xs, dw, c.R, c.R, c.stride, c.pad, c.dil, splits=splits, qscale=qs)
        else:
            HF.conv2d_wgrad(self.dys[0], self.xs[0], dw, c.R, c.R, c.stride, c.pad, c.dil, splits=splits, qscale=qs, side=False)

    def host(self, dw):
        dw = dw.cpu()
        return self.module.window_blocks(dw) if self.module is not None else dw

    def run(self, name, tag, splits, want, out):
        """Into zeros, once more into the result (compared as dw / 2), with qscale; every dispatch must be kernel ``want``."""
        dw, guard = R.guarded(self.shape, torch.float32, self.cuda, fill=0.0)
        dq, qguard = R.guarded(self.shape, torch.float32, self.cuda, fill=0.0)
        res = {}

        def go():
            self.launch(dw, splits)
            torch.cuda.synchronize()
            res["first"] = dw.clone()
            self.launch(dw, splits)
            self.launch(dq, splits, qscale=True)

        seen = _wgrad_variants(go)
        assert seen == [want] * 3, (name, tag, "weight-gradient dispatches ran on %s, the case is about %d" % (seen, want))
        R.assert_guards_intact(guard, name + " dW")
        R.assert_guards_intact(qguard, name + " dW qscale")
        out[tag] = R.check(self.host(res["first"]), *_wg_ref(name, False), False, enforce=False)
        out[tag + " x2"] = R.check(self.host(dw) / 2, *_wg_ref(name, False), False, enforce=False)
        out[tag + " qscale"] = R.check(self.host(dq), *_wg_ref(name, True), False, enforce=False)
        return res["first"]


# kernel of the case table -> [(tag, knobs, splits, variant code)]
_WGRAD_RUNS = {
    "w128": [("splits1", {"sod_conv_set_wgrad_variant": 0}, 1, W128), ("splits3", {"sod_conv_set_wgrad_variant": 0}, 3, W128),
             ("ring2300", {"sod_conv_set_wgrad_variant": 2300}, "own", 2300), ("ring2310 splits3", {"sod_conv_set_wgrad_variant": 2310}, 3, 2310)],
    "ring": [("ring2300", {"sod_conv_set_wgrad_variant": 2300}, 0, 2300), ("ring2310", {"sod_conv_set_wgrad_variant": 2310}, 0, 2310)],
    "w256": [("wgrad256", {}, -1, W256)],
    "w9": [("wgrad9", {}, -2, W9)],
    "fold": [("fold", {}, 0, WFOLD), ("unfolded splits3", {}, 3, W128)],
    "diag": [("diag", {}, 0, W128)],
}


def _fold_takes(c):
    """wgrad_fold_supported (conv_wgrad_fold.hip): with ``splits=0`` these shapes go to the folded kernel BEFORE the variant knob is
    looked at (3x3 with K = 64 / 72 do), so the ring kernel is reached with an explicit split count only."""
    same = all(R.out_size(h, w, c.R, c.R, c.stride, c.pad, c.dil) == (h, w) for h, w in c.levels)
    taps = c.R * c.R
    return c.stride == 1 and c.K % 8 == 0 and taps > 1 and same and -(-taps * c.K // 128) * 3 <= taps * -(-c.K // 128) * 2


@pytest.mark.parametrize("name", list(R.WGRAD_CASES))
def test_weight_gradient_per_element(cuda, name):
    c = _wg_case(name)
    dev = _WDev(c, cuda)
    out = {}
    for tag, knobs, splits, want in _WGRAD_RUNS[c.kernel]:
        if splits == "own":                                 # the dispatcher's own split count where the ring kernel is reached with it
            splits = 2 if _fold_takes(c) else 0
            tag += " splits%d" % splits
        with _knobs(knobs):
            first = dev.run(name, tag, splits, want, out)
            if want in (W256, W9, 2310):                    # slabs summed in a fixed order: bit-identical from run to run
                again = torch.zeros_like(first)
                dev.launch(again, splits)
                torch.cuda.synchronize()
                assert torch.equal(again, first), (name, tag)
    _assert_all("wgrad " + name, out)


# one case per kernel that honours the deterministic mode: (case, knobs, splits, variant code)
_DET_RUNS = [("w128_c136_k72", {"sod_conv_set_wgrad_variant": -1}, 0, W128), ("w128_s2", {"sod_conv_set_wgrad_variant": 2300}, 0, 2310),
             ("ring_3lev", {"sod_conv_set_wgrad_variant": 2300}, 0, 2310), ("w256_k264_1x1", {}, -1, W256), ("w9_k136", {}, -2, W9),
             ("diag_s2", {}, 0, W128)]


@pytest.mark.parametrize("name,knobs,splits,want", _DET_RUNS, ids=[r[0] + "-%d" % r[3] for r in _DET_RUNS])
def test_deterministic_mode_per_element(cuda, name, knobs, splits, want):
    """HF.DETERMINISTIC: bit-identical repeats AND the per-element bound (the ring kernel then takes its slab epilogue, 2310)."""
    from slenderobjdet_amd.layers import functional as HF

    dev = _WDev(_wg_case(name), cuda)
    out = {}
    prev, HF.DETERMINISTIC = HF.DETERMINISTIC, True
    try:
        with _knobs(knobs):
            first = dev.run(name, "det", splits, want, out)
            again = torch.zeros_like(first)
            dev.launch(again, splits)
            torch.cuda.synchronize()
    finally:
        HF.DETERMINISTIC = prev
    assert torch.equal(again, first), (name, "deterministic mode: two runs differ")
    _assert_all("wgrad " + name + " deterministic", out)
