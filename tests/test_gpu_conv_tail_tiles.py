"""Remainder tiles of a split conv dispatch (csrc/conv_dispatch.hip: whole rounds of pixel tiles on the 256x256 kernel, the rest in a
second launch of the 128x128-family kernel, sod_conv_set_tail_tile).

sod_conv_set_tail_split(n) splits every dispatch the 256x256 kernel supports after its first n 256-pixel tiles, so that tiny shapes
take the main + remainder path.  For each remainder tile (64x64, 64x128, 64x64 with three LDS ring slots), forward and data gradient:

  * bit identity (torch.equal on the whole output) with the remainder on the 128x128 tile (sod_conv_set_tail_tile(0)): every tile
    produces an output element with the same MFMA instruction and K order;
  * the same outputs against F.conv2d / its gradient in float64 on bf16-rounded operands, at the bounds of tests/test_gpu_conv.py:
    2^-7 * max|ref| for bf16 outputs, 2e-4 * max|ref| for fp32 outputs;
  * the GroupNorm statistics of sod_conv2d_fwd_ml_gnsum (float atomics, so not bit-identical) against float64 sums of the stored
    outputs at the mean / rstd bounds of tests/test_gpu_groupnorm.py (EPS_M * max|x| of the group, EPS_R relative).

Cases: 256 -> 256 3x3, N = 2, levels 16x24 + 5x7 split after 2 tiles (pstart = 512 inside level 0 - a multiple of 256, not of the row
length 24 -, level 1 wholly remainder); 1024 -> 256 1x1, N = 1, 19x23 split after 1 tile (181 remainder pixels: no multiple of 64);
256 -> 256 3x3, N = 1, 18x22 with the half-resolution residual; 1024 -> 256 1x1, N = 1, 8x37 split after 1 tile (40 remainder pixels:
one partial tile of every shape).  Epilogues: bias + ReLU, residual (+ ReLU), up-sampled residual, fp32 output, ReLU mask, accumulate + mask,
GroupNorm statistics.

Host side (no GPU): the selection rule on the split dispatches of the FCOS R50 step through sod_conv_plan / sod_conv_tail_tile_select.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

T128, T64x128, T64x64, T64x64_R3 = 12812864, 6412864, 6406464, 36406464
NEW_TILES = [T64x64, T64x128, T64x64_R3]
BF16, F32 = 2 ** -7, 2e-4


def _rb(t):
    return t.bfloat16().float()


def _rand(shape, seed, scale=1.0):
    return _rb(torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale)


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv64(x, w, b, pad):
    return _nhwc(F.conv2d(_nchw(x), w.double().permute(0, 3, 1, 2), None if b is None else b.double(), 1, pad))


def _dgrad64(dy, w, hw, pad):
    x = torch.zeros(dy.shape[0], w.shape[3], *hw, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w.double().permute(0, 3, 1, 2), None, 1, pad)
    (gx,) = torch.autograd.grad(y, x, _nchw(dy))
    return _nhwc(gx)


def _up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


# ---- the operations under test: name -> (split point, inputs(), run(HF, cuda-side inputs) -> [outputs], ref(inputs) -> [float64], [bounds]) ----

LEVELS = [(16, 24), (5, 7)]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    if name.startswith("ml_"):      # 256 -> 256 3x3, N = 2, two levels
        d = {"x": [_rand((2, h, w, 256), 10 + i) for i, (h, w) in enumerate(LEVELS)], "w": _rand((256, 3, 3, 256), 2, 0.05),
             "b": torch.randn(256, generator=torch.Generator().manual_seed(3)),
             "dy": [_rand((2, h, w, 256), 20 + i) for i, (h, w) in enumerate(LEVELS)],
             "mask": [_rand((2, h, w, 256), 30 + i) for i, (h, w) in enumerate(LEVELS)],
             "acc": [_rand((2, h, w, 256), 40 + i) for i, (h, w) in enumerate(LEVELS)]}
    elif name.startswith("pw_") or name.startswith("one_"):      # 1024 -> 256 1x1, N = 1
        H, W = (19, 23) if name.startswith("pw_") else (8, 37)
        d = {"x": _rand((1, H, W, 1024), 50), "w": _rand((256, 1, 1, 1024), 51, 0.05), "b": torch.randn(256, generator=torch.Generator().manual_seed(52)),
             "res": _rand((1, H, W, 256), 53), "dy": _rand((1, H, W, 256), 54), "mask": _rand((1, H, W, 1024), 55), "acc": _rand((1, H, W, 1024), 56)}
    else:      # up2_: 256 -> 256 3x3, N = 1, 18x22, residual at half resolution
        d = {"x": _rand((1, 18, 22, 256), 60), "w": _rand((256, 3, 3, 256), 61, 0.05), "b": torch.randn(256, generator=torch.Generator().manual_seed(62)),
             "prev": _rand((1, 9, 11, 256), 63)}
    return d


def _dev(v, cuda, dtype=torch.bfloat16):
    if isinstance(v, list):
        return [_dev(t, cuda, dtype) for t in v]
    return v.to(cuda).to(dtype)


def _wt(HF, w, cuda):
    return HF.weight_prep(w.to(cuda), want_krsc=False)[1]


def _gnsum(HF, xs, w, b, cuda):
    """sod_conv2d_fwd_ml_gnsum as layers/functional.conv_gn_fwd_ml calls it, without the apply pass: (outputs, raw sums (nlev, N, G, 2))."""
    N, K, G = xs[0].shape[0], w.shape[0], w.shape[0] // 8
    hs, ws = [x.shape[1] for x in xs], [x.shape[2] for x in xs]
    outs = [torch.empty((N, h, wd, K), dtype=torch.bfloat16, device=cuda) for h, wd in zip(hs, ws)]
    sums = torch.full((len(xs), N, G, 2), 7.0, dtype=torch.float32, device=cuda)      # the call zeroes them
    HF.call("sod_conv2d_fwd_ml_gnsum", len(xs), HF._ptr_arr(xs), HF.ptr(w), HF.ptr(b), HF._ptr_arr(outs), N, HF._int_arr(hs), HF._int_arr(ws),
            w.shape[3], K, 3, 3, 1, 1, 1, 0, 0, HF.ptr(sums), G, HF.stream_ptr())
    return outs, sums


def _run(name, HF, cuda):
    d = _inputs(name)
    if name == "ml_fwd_bias_relu":
        return HF.conv2d_fwd_ml(_dev(d["x"], cuda), _dev(d["w"], cuda), d["b"].to(cuda), 1, 1, 1, relu=True)
    if name == "ml_fwd_gnsum":
        outs, sums = _gnsum(HF, _dev(d["x"], cuda), _dev(d["w"], cuda), d["b"].to(cuda), cuda)
        return outs + [sums]
    if name == "ml_dgrad_mask":
        return HF.conv2d_dgrad_ml(_dev(d["dy"], cuda), _wt(HF, d["w"], cuda), LEVELS, 1, 1, 1, relu_masks=_dev(d["mask"], cuda))
    if name == "ml_dgrad_accum_mask":
        return HF.conv2d_dgrad_ml(_dev(d["dy"], cuda), _wt(HF, d["w"], cuda), LEVELS, 1, 1, 1, relu_masks=_dev(d["mask"], cuda), accums=_dev(d["acc"], cuda))
    if name in ("pw_fwd_res_relu", "one_fwd_res_relu"):
        return [HF.conv2d_fwd(_dev(d["x"], cuda), _dev(d["w"], cuda), d["b"].to(cuda), res=_dev(d["res"], cuda), relu=True)]
    if name == "pw_fwd_f32":
        return [HF.conv2d_fwd(_dev(d["x"], cuda), _dev(d["w"], cuda), d["b"].to(cuda), out_f32=True)]
    if name in ("pw_dgrad_accum_mask", "one_dgrad_accum_mask"):
        hw = tuple(d["dy"].shape[1:3])
        return [HF.conv2d_dgrad(_dev(d["dy"], cuda), _wt(HF, d["w"], cuda), hw, 1, 0, 1, accum=_dev(d["acc"], cuda), relu_mask=_dev(d["mask"], cuda))]
    if name == "up2_fwd_res":
        return [HF.conv2d_fwd(_dev(d["x"], cuda), _dev(d["w"], cuda), d["b"].to(cuda), res=_dev(d["prev"], cuda), pad=1, res_up2=True)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    d = _inputs(name)
    if name in ("ml_fwd_bias_relu", "ml_fwd_gnsum"):
        ys = [_conv64(x, d["w"], d["b"], 1) for x in d["x"]]
        return [y.relu() for y in ys] if name == "ml_fwd_bias_relu" else ys
    if name == "ml_dgrad_mask":
        return [_dgrad64(dy, d["w"], hw, 1) * (m > 0) for dy, hw, m in zip(d["dy"], LEVELS, d["mask"])]
    if name == "ml_dgrad_accum_mask":
        return [(_dgrad64(dy, d["w"], hw, 1) + a.double()) * (m > 0) for dy, hw, m, a in zip(d["dy"], LEVELS, d["mask"], d["acc"])]
    if name in ("pw_fwd_res_relu", "one_fwd_res_relu"):
        return [(_conv64(d["x"], d["w"], d["b"], 0) + d["res"].double()).relu()]
    if name == "pw_fwd_f32":
        return [_conv64(d["x"], d["w"], d["b"], 0)]
    if name in ("pw_dgrad_accum_mask", "one_dgrad_accum_mask"):
        return [(_dgrad64(d["dy"], d["w"], tuple(d["dy"].shape[1:3]), 0) + d["acc"].double()) * (d["mask"] > 0)]
    if name == "up2_fwd_res":
        return [_conv64(d["x"], d["w"], d["b"], 1) + _up2(d["prev"]).double()]
    raise KeyError(name)


# name: (main tiles before the split, forward?)
OPS = {
    "ml_fwd_bias_relu": (2, True), "ml_fwd_gnsum": (2, True), "ml_dgrad_mask": (2, False), "ml_dgrad_accum_mask": (2, False),
    "pw_fwd_res_relu": (1, True), "pw_fwd_f32": (1, True), "pw_dgrad_accum_mask": (1, False),
    "up2_fwd_res": (1, True), "one_fwd_res_relu": (1, True), "one_dgrad_accum_mask": (1, False),
}
_base = {}


def _with_tail(name, tile, cuda):
    """The op with the split forced and the remainder on `tile` (0 = the ordinary 128x128 remainder) -> outputs on the CPU."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    _C.call("sod_conv_set_tail_split", OPS[name][0])
    _C.call("sod_conv_set_tail_tile", tile)
    try:
        outs = _run(name, HF, cuda)
        lib = _C.load()
        assert int(lib.sod_conv_last_variant()) == 256, "the dispatch did not take the 256x256 kernel + remainder path"
        assert int(lib.sod_conv_last_tail_variant()) == (tile or T128)
        torch.cuda.synchronize()
    finally:
        _C.call("sod_conv_set_tail_split", -1)
        _C.call("sod_conv_set_tail_tile", -1)
    return [o.cpu() for o in outs]


def _close(got, ref, rel, what):
    tol = rel * max(ref.abs().max().item(), 1e-6)
    err = (got.double() - ref).abs().max().item()
    print(f"{what}: max abs err {err:.4g}, bound {tol:.4g}")
    assert err <= tol, f"{what}: max abs err {err:.4g} > tol {tol:.4g} (ref max {ref.abs().max().item():.4g})"


def _check_gn_sums(sums, ys, what):
    """(sum, sum of squares) per (level, image, group) of the STORED outputs ys, as mean / rstd at the bounds of tests/test_gpu_groupnorm.py."""
    from test_gpu_groupnorm import EPS_M, EPS_R

    for l, y in enumerate(ys):
        N, H, W, K = y.shape
        g = y.double().reshape(N, H * W, K // 8, 8)
        cnt = H * W * 8
        mean = g.sum(dim=(1, 3)) / cnt
        rstd = 1.0 / torch.sqrt((g * g).sum(dim=(1, 3)) / cnt - mean * mean + 1e-5)
        m = sums[l, :, :, 0].double() / cnt
        r = 1.0 / torch.sqrt(sums[l, :, :, 1].double() / cnt - m * m + 1e-5)
        em = ((m - mean).abs() / g.abs().amax(dim=(1, 3))).max().item()
        er = ((r - rstd).abs() / rstd).max().item()
        print(f"{what} level {l}: mean err {em:.3g} of max|x| (bound {EPS_M:.3g}), rstd rel err {er:.3g} (bound {EPS_R:.3g})")
        assert em <= EPS_M and er <= EPS_R, (what, l, em, er)


@gpu
@pytest.mark.parametrize("tile", NEW_TILES)
@pytest.mark.parametrize("name", list(OPS))
def test_tail_tile_bit_identical_and_float64(cuda, name, tile):
    if name not in _base:
        _base[name] = _with_tail(name, 0, cuda)
    base, got, ref = _base[name], _with_tail(name, tile, cuda), _ref(name)
    nout = len(ref)
    for l in range(nout):
        assert got[l].dtype == base[l].dtype and torch.equal(got[l], base[l]), f"{name} tile {tile} output {l}: differs from the 128x128 remainder"
        _close(got[l], ref[l], F32 if got[l].dtype == torch.float32 else BF16, f"{name} tile {tile} output {l}")
    if name == "ml_fwd_gnsum":
        _check_gn_sums(base[nout], base[:nout], f"{name} 128x128 remainder")
        _check_gn_sums(got[nout], got[:nout], f"{name} tile {tile}")


@gpu
def test_forced_tile_leaves_other_dispatches_alone(cuda):
    """A dispatch that is not split runs on the same kernel whatever the remainder knob says; an unknown tile code is rejected."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    x, w = _dev(_rand((2, 13, 21, 64), 1), cuda), _dev(_rand((128, 3, 3, 64), 2, 0.05), cuda)
    x2, w2 = _dev(_inputs("up2_fwd_res")["x"], cuda), _dev(_inputs("up2_fwd_res")["w"], cuda)
    seen = []
    try:
        for mode in (0, 1, T64x64):
            _C.call("sod_conv_set_tail_tile", mode)
            y = HF.conv2d_fwd(x, w, None, stride=1, pad=1)
            v = int(_C.load().sod_conv_last_variant())
            y2 = HF.conv2d_fwd(x2, w2, None, stride=1, pad=1)      # 256-capable, but far below one round: not split
            seen.append((v, int(_C.load().sod_conv_last_tail_variant()), int(_C.load().sod_conv_last_variant()), y.cpu(), y2.cpu()))
        assert _C.load().sod_conv_set_tail_tile(12812832) == -1 and _C.load().sod_conv_set_tail_tile(2) == -1
    finally:
        _C.call("sod_conv_set_tail_tile", -1)
    for s in seen[1:]:
        assert s[:3] == seen[0][:3] and s[1] == 0 and torch.equal(s[3], seen[0][3]) and torch.equal(s[4], seen[0][4])


# ---- host side ----

def _plan(lib, mode, N, hws, C, K, R, stride=1):
    n = len(hws)
    H, W = (ctypes.c_int * n)(*[h for h, _ in hws]), (ctypes.c_int * n)(*[w for _, w in hws])
    tv, mp = ctypes.c_int(-1), ctypes.c_int(-1)
    v = lib.sod_conv_plan(mode, n, N, ctypes.cast(H, ctypes.c_void_p), ctypes.cast(W, ctypes.c_void_p), C, K, R, R, stride, R // 2, 1,
                          ctypes.byref(tv), ctypes.byref(mp))
    return v, tv.value, mp.value


FPN = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
# (mode, levels of the convolution's input side, C, K, R): the split dispatches of the FCOS R50 step at batch 16, 800 x 1344
R50_SPLIT = [
    (0, [(50, 84)], 1024, 256, 1),      # res4 conv1 (blocks 2..6) / lateral C4
    (0, [(50, 84)], 256, 256, 3),       # res4 conv2 / output P4
    (1, [(50, 84)], 256, 1024, 1),      # res4 conv3 data gradient
    (1, [(50, 84)], 256, 256, 3),       # res4 conv2 / output P4 data gradient
    (0, [(100, 168)], 256, 256, 3),     # output P3
    (1, [(100, 168)], 256, 256, 3),
]
R50_TOWER = [(0, FPN, 256, 256, 3), (1, FPN, 256, 256, 3)]
# not split: on the 128x128-family tiles, the persistent kernels, or the 256x256 kernel with a remainder of half a round or more
R50_OTHER = [(0, [(25, 42)], 2048, 512, 1), (0, [(25, 42)], 512, 512, 3), (0, [(100, 168)], 512, 256, 1), (0, FPN, 256, 80, 3), (0, FPN, 256, 8, 3),
             (1, FPN, 256, 80, 3), (0, [(100, 168)], 128, 128, 3), (0, [(100, 168)], 128, 512, 1), (0, [(13, 21)], 256, 256, 3)]


def test_selection_rule_host():
    from slenderobjdet_amd import _C

    lib = _C.load()
    supported = {T128, T64x128, T64x64, T64x64_R3}
    try:
        assert lib.sod_conv_set_tail_tile(1) == 0 and lib.sod_conv_set_tail_split(0) == 0 and lib.sod_conv_set_tile256(1) == 0
        # the towers' 122-tile remainder keeps the 128x128 tile
        for case in R50_TOWER:
            v, tail, main = _plan(lib, case[0], 16, case[1], *case[2:])
            assert (v, tail, main) == (256, T128, 1280), (case, v, tail, main)
        assert lib.sod_conv_tail_tile_select(122 * 256, 256, 2304, 256) == T128
        for case in R50_SPLIT:
            v, tail, main = _plan(lib, case[0], 16, case[1], *case[2:])
            assert v == 256 and tail in supported and main in (256, 1024), (case, v, tail, main)
        # every remainder below half a round gets a supported tile
        for kred in (1024, 2304):
            for nout in (256, 1024):
                for rem in range(1, 128):
                    assert lib.sod_conv_tail_tile_select(rem * 256, nout, kred, 256) in supported, (rem, nout, kred)
        assert lib.sod_conv_tail_tile_select(0, 256, 1024, 256) == -1
        # no other dispatch changes its kernel with the knob, and the main launch of a split one never does
        plans = {}
        for mode in (0, 1, T64x64, T64x128, T64x64_R3, T128):
            assert lib.sod_conv_set_tail_tile(mode) == 0
            plans[mode] = [_plan(lib, c[0], 16, c[1], *c[2:]) for c in R50_OTHER + R50_SPLIT + R50_TOWER]
        for mode, p in plans.items():
            for case, a, b in zip(R50_OTHER + R50_SPLIT + R50_TOWER, p, plans[0]):
                assert a[0] == b[0] and a[2] == b[2], (mode, case, a, b)
                if case in R50_OTHER:
                    assert a == b and a[1] == 0, (mode, case, a, b)
                elif mode > 1:
                    assert a[1] == mode, (mode, case, a)
                elif mode == 0:
                    assert a[1] == T128, (case, a)
    finally:
        lib.sod_conv_set_tail_tile(-1)
        lib.sod_conv_set_tail_split(-1)
        lib.sod_conv_set_tile256(-1)
