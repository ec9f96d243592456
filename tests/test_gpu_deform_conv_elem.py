"""The deformable-convolution kernels (csrc/deform_conv.hip, csrc/dcn_fused.hip) against the float64 restatement of
tests/deform_conv_restated.py, PER ELEMENT and with no element left out: every bound is the restatement's (derived there from the
number formats, the number of addends, the absolute-addend sums and the kernels' fixed-point quantum; nothing is tuned to what
the kernels give).  tests/test_deform_conv_restated_host.py shows on the CPU that the same checks pass a correct fp32 / bf16
emulation and reject eight kinds of wrong answer, for every case used here.

Which case reaches which kernel (from the launchers' conditions):

* forward: ``deform_im2col`` -> dcn_im2col_kernel<bf16>; + ``conv2d_fwd`` (bf16 and out_f32); ``deform_conv_fwd_fused`` ->
  dcn_fwd_fused_kernel (K = 264: second q tile of 8 channels; P = 1, 128, 129: one / exactly one / two 128-pixel tiles);
  ``deform_conv_fwd_f32`` -> dcn_fwd_f32_kernel.
* ``deform_col2im``: cpg % 32 != 0 or a window above 64 KB -> dcn_col2im_kernel<bf16> (plain_c64_dg4: red = 2, plain_c64_s2:
  red = 8, plain_c48 / plain_c96_dg2: red = 0, float atomics); else dcn_col2im_tile_kernel<32> (tiled_*: 3x3, 1x1 at stride 1 and 2,
  5x5; fbits 20 / 24 / 19).  ``sod_deform_col2im_f32`` -> dcn_col2im_kernel<float> (C = 16: red = 2, C = 48: red = 0).
* ``deform_conv_bwd_fused`` -> dcn_bwd_fused_kernel<KS, GM, STG>: KS = K / 32 (4, 8, 16), GM = a mask gradient is wanted, STG = 4 px of
  slack with at most nine taps (5x5 at 4 px takes the non-staged kernel); C = 32 is a single channel chunk.
"""
import functools

import pytest
import torch

import deform_conv_restated as D

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(table, name):
    c = D.case(getattr(D, table), name)
    f = D.forward(c.x, c.R, c.w, c.mask, c.logit, c.bias)
    b = D.backward(c.x, c.R, c.w, c.dy, c.mask, c.logit)
    return c, f, b


def _show(name, out):
    print("RATIO", name, {k: "%.3f" % v["ratio"] for k, v in out.items()})


class _Dev:
    """The case's tensors on the device, in the kernels' formats (offsets / mask in pitched buffers where the case asks for it)."""

    def __init__(self, c, cuda):
        from slenderobjdet_amd.layers import functional as HF

        assert c.R.floors_agree                # fp32-formed positions floor like the exact sums: no element needs leaving out
        self.ld = c.ld or 0
        self.x = c.x.to(cuda) if c.f32 else c.x.to(cuda).bfloat16()
        self.off = (D.pitched(c.off, self.ld) if self.ld else c.off).to(cuda)
        self.mask = None if c.mask is None else (D.pitched(c.mask, self.ld) if self.ld else c.mask).to(cuda)
        self.dy = c.dy.to(cuda) if c.f32 else c.dy.to(cuda).bfloat16()
        self.bias = c.bias.to(cuda)
        self.w_flat = c.w.reshape(c.K, 1, 1, c.taps * c.C).to(cuda)
        if not c.f32:
            self.wk, self.wt = HF.weight_prep(self.w_flat)
        self.geo = (c.ksize, c.stride, c.pad, c.dil, c.dg)

    def grads(self):
        return torch.zeros_like(self.off), None if self.mask is None else torch.zeros_like(self.mask)


def _padding_is_zero(t, n):
    return t is None or t.shape[-1] == n or float(t[..., n:].abs().max()) == 0.0


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(D.FWD_CASES))
def test_forward_per_element(cuda, name):
    from slenderobjdet_amd.layers import functional as HF

    c, f, _ = _case("FWD_CASES", name)
    d = _Dev(c, cuda)
    paths = c.paths or ("cols", "gemm", "fused")
    kw = dict(off_ld=d.ld, mask_ld=d.ld, mask_is_logit=c.logit)
    out = {}
    if "f32" in paths:
        y = HF.deform_conv_fwd_f32(d.x, d.off, d.mask, d.w_flat.reshape(c.K, -1), d.bias, *d.geo, mask_is_logit=c.logit)
        out["fwd_f32"] = D.check_fwd(y.cpu(), f, "f32", enforce=False)
    cols = None
    if "cols" in paths or "gemm" in paths:
        cols = HF.deform_im2col(d.x, d.off, d.mask, *d.geo, **kw)
        out["im2col"] = D.check_cols(cols.float().cpu(), f, enforce=False)
    if "gemm" in paths:
        out["cols+gemm f32"] = D.check_fwd(HF.conv2d_fwd(cols, d.wk, d.bias, stride=1, pad=0, out_f32=True).cpu(), f, "out_f32", enforce=False)
        out["cols+gemm bf16"] = D.check_fwd(HF.conv2d_fwd(cols, d.wk, d.bias, stride=1, pad=0).float().cpu(), f, "bf16", enforce=False)
    if "fused" in paths:
        fr = D.forward(c.x, c.R, c.w, c.mask, c.logit, c.bias, relu=True)
        y = HF.deform_conv_fwd_fused(d.x, d.off, d.mask, d.wk, d.bias, *d.geo, relu=True, **kw)
        assert tuple(y.shape) == (c.N, c.Ho, c.Wo, c.K)
        out["fused relu"] = D.check_fwd(y.float().cpu(), fr, "bf16", enforce=False)
        y = HF.deform_conv_fwd_fused(d.x, d.off, d.mask, d.wk, None, *d.geo, **kw)
        out["fused"] = D.check_fwd(y.float().cpu(), D.forward(c.x, c.R, c.w, c.mask, c.logit), "bf16", enforce=False)
    _show(name, out)
    for k, v in out.items():
        assert v["same_nonfinite"] and v["ratio"] <= 1.0 and v["compared"] > 0, (k, v)


# ------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("name", list(D.WGRAD_CASES))
def test_weight_gradient_per_element(cuda, name):
    from slenderobjdet_amd.layers import functional as HF

    c, _, b = _case("WGRAD_CASES", name)
    d = _Dev(c, cuda)
    scale = 2.0 ** (torch.arange(c.K) % 5 - 2).float() if c.qscale else None          # powers of two: the bound scales exactly
    qs = scale.to(cuda) if c.qscale else None
    kw = dict(mask_is_logit=c.logit)

    def run():
        dw = torch.zeros(c.K, 1, 1, c.taps * c.C, device=cuda)
        HF.deform_conv_wgrad_fused(d.dy, d.x, d.off, d.mask, dw, *d.geo, qscale=qs, **kw)
        HF.wgrad_join()
        torch.cuda.synchronize()
        return dw

    dw = run()
    shape = (c.K, c.taps, c.C)
    out = {"wgrad fused": D.check_dw(dw.cpu().reshape(shape), b, scale=scale, enforce=False)}
    cols = HF.deform_im2col(d.x, d.off, d.mask, *d.geo, **kw)
    dw_cols = torch.zeros_like(dw)
    HF.conv2d_wgrad(d.dy, cols, dw_cols, 1, 1, 1, 0, 1, qscale=qs)
    HF.wgrad_join()
    torch.cuda.synchronize()
    out["wgrad cols"] = D.check_dw(dw_cols.cpu().reshape(shape), b, scale=scale, enforce=False)
    first = dw.clone()
    HF.deform_conv_wgrad_fused(d.dy, d.x, d.off, d.mask, dw, *d.geo, qscale=qs, **kw)       # accumulates into dW
    HF.wgrad_join()
    torch.cuda.synchronize()
    out["wgrad fused x2"] = D.check_dw(dw.cpu().reshape(shape) / 2, b, scale=scale, enforce=False)
    _show(name, out)
    for k, v in out.items():
        assert v["same_nonfinite"] and v["ratio"] <= 1.0, (k, v)
    assert torch.equal(run(), first)                                                         # fixed summation order


# ------------------------------------------------------------------ input / offset / mask gradients
def _col2im(HF, c, d, dcols_dev, f32=False):
    doff, dmask = d.grads()
    if f32:
        dx = torch.zeros(c.N, c.H, c.W, c.C, device=dcols_dev.device)
        HF.call("sod_deform_col2im_f32", HF.ptr(dcols_dev), HF.ptr(d.x), HF.ptr(d.off), HF.ptr(d.mask), HF.ptr(dx), HF.ptr(doff), HF.ptr(dmask), c.N, c.H, c.W,
                c.C, c.ksize[0], c.ksize[1], c.stride, c.pad, c.dil, c.dg, d.ld, d.ld, 1 if c.logit else 0, HF.stream_ptr())
    else:
        dx = HF.deform_col2im(dcols_dev, d.x, d.off, d.mask, *d.geo, doff, dmask, off_ld=d.ld, mask_ld=d.ld, mask_is_logit=c.logit)
    return dx, doff, dmask


def _check_grads(c, b, dx, doff, dmask, qsum, mode, tag):
    out = {tag + " dx": D.check_dx(dx.cpu(), b, qsum, mode, enforce=False), tag + " doff": D.check_doff(doff.cpu(), b, mode, enforce=False)}
    if c.mask is not None:
        out[tag + " dmask"] = D.check_dmask(dmask.cpu(), b, mode, enforce=False)
    assert _padding_is_zero(doff, 2 * c.taps * c.dg) and _padding_is_zero(dmask, c.taps * c.dg)
    return out


def _assert_all(name, out):
    _show(name, out)
    for k, v in out.items():
        assert v["same_nonfinite"], (k, "non-finite elements are not the reference's")
        assert v["ratio"] <= 1.0, (k, v)


def _fused_at_slacks(HF, c, d, b, qsum, tag="fused"):
    out = {}
    for slack in (2, 4):
        HF.call("sod_deform_conv_set_window_slack", slack)
        try:
            if not HF.deform_bwd_fused_supported(c.C, c.K, c.dg, c.ksize, c.stride, c.dil):
                assert slack == 4                       # every case fits at the default slack
                continue
            doff, dmask = d.grads()
            dx = HF.deform_conv_bwd_fused(d.dy, d.wt, d.x, d.off, d.mask, *d.geo, doff, dmask, off_ld=d.ld, mask_ld=d.ld, mask_is_logit=c.logit)
            torch.cuda.synchronize()
        finally:
            HF.call("sod_deform_conv_set_window_slack", -1)
        out.update(_check_grads(c, b, dx, doff, dmask, qsum, "bf16", "%s slack %d" % (tag, slack)))
    return out


@pytest.mark.parametrize("name", list(D.BWD_CASES))
def test_input_offset_mask_gradients_per_element(cuda, name):
    from slenderobjdet_amd.layers import functional as HF

    c, _, b = _case("BWD_CASES", name)
    d = _Dev(c, cuda)
    if c.path == "fused":
        qsum = D.dx_quantum_sum(D.quantum_fused(c.dy, c.w, c.R, c.mask, c.logit), c.R)
        out = _fused_at_slacks(HF, c, d, b, qsum)
    elif c.path == "f32":
        dc = b.dcols.float()                                  # the kernel's input: the reference takes exactly these column gradients
        b32 = D.backward(c.x, c.R, None, None, c.mask, c.logit, dcols=dc)
        out = _check_grads(c, b32, *_col2im(HF, c, d, dc.to(cuda), f32=True), None, "f32", "col2im f32")
    else:
        dc = D.rb(b.dcols.float())                            # what the 1x1 data gradient stores
        qsum = D.dx_quantum_sum(D.quantum_tiled(dc, c.R, c.mask, c.logit), c.R) if c.path == "tiled" else None
        out = _check_grads(c, b, *_col2im(HF, c, d, dc.to(cuda).bfloat16()), qsum, "bf16", "col2im " + c.path)
    _assert_all(name, out)


# ------------------------------------------------------------------ adversarial fixed-point cases
V, S = 0.4375, 1.0 / 32          # dY[p, k] = +-V, W[k, tap, c] = S * dY[p, k]: bf16 values, dcols = K V^2 S exactly = the Cauchy-Schwarz bound


@pytest.mark.parametrize("kernel", ["tiled", "fused"])
@pytest.mark.parametrize("k", [3, 5])
def test_every_contribution_of_a_tile_in_one_cell(cuda, kernel, k):
    """(i) all 64 * taps samples of an 8x8 tile land exactly on input pixel (3, 3) with the same sign (576 for 3x3, 1600 for 5x5):
    the no-overflow argument of the int32 window at its limit; in the fused kernel dY is parallel to every weight column, so the
    Cauchy-Schwarz bound the scale comes from is attained."""
    from slenderobjdet_amd.layers import functional as HF

    K, C = 128, 32
    c = D.make_case(1, C, K, 8, 8, ksize=(k, k), pad=k // 2, program="converge", seed=77 + k)
    c.ld = None
    sign = 1.0 - 2.0 * (torch.arange(K) % 2)
    c.dy = (V * sign).expand(1, 8, 8, K).contiguous()
    c.w = (S * V * sign).view(K, 1, 1).expand(K, c.taps, C).contiguous()
    assert bool((D.rb(c.dy) == c.dy).all()) and bool((D.rb(c.w) == c.w).all())
    d = _Dev(c, cuda)
    b = D.backward(c.x, c.R, c.w, c.dy)
    each = K * V * V * S
    assert float((b.dcols - each).abs().max()) == 0 and D.rb(torch.tensor(each)).item() == each
    assert float(b.dxn[0, 3, 3].min()) == 64 * c.taps and float((b.dx[0, 3, 3] - 64 * c.taps * each).abs().max()) == 0
    if kernel == "tiled":
        dc = b.dcols.float()
        qsum = D.dx_quantum_sum(D.quantum_tiled(dc, c.R), c.R)
        out = _check_grads(c, b, *_col2im(HF, c, d, dc.to(cuda).bfloat16()), qsum, "bf16", "tiled")
    else:
        out = _fused_at_slacks(HF, c, d, b, D.dx_quantum_sum(D.quantum_fused(c.dy, c.w, c.R), c.R))
    _assert_all("converge %dx%d %s" % (k, k, kernel), out)


def _two_tile_case(seed, mask):
    c = D.make_case(1, 64, 128, 8, 16, program="random", spread=4.3, mask=mask, seed=seed)
    c.ld = None
    return c


def _run_both(HF, cuda, c, b, tag):
    d = _Dev(c, cuda)
    dc = D.rb(b.dcols.float())
    out = _check_grads(c, b, *_col2im(HF, c, d, dc.to(cuda).bfloat16()), D.dx_quantum_sum(D.quantum_tiled(dc, c.R, c.mask, c.logit), c.R), "bf16", "tiled")
    out.update(_fused_at_slacks(HF, c, d, b, D.dx_quantum_sum(D.quantum_fused(c.dy, c.w, c.R, c.mask, c.logit), c.R)))
    _assert_all(tag, out)
    return d


def test_adjacent_tiles_with_scales_2_to_the_20_apart(cuda):
    """(ii) the right tile's dY is 2^-20 of the left one's; their windows overlap on the same dx pixels.  Each tile's contributions are
    held to its OWN quantum: a cell only the small tile reaches has a bound 2^20 times smaller."""
    from slenderobjdet_amd.layers import functional as HF

    c = _two_tile_case(501, "rand")
    c.dy[:, :, 8:] *= 2.0 ** -20
    b = D.backward(c.x, c.R, c.w, c.dy, c.mask, c.logit)
    _run_both(HF, cuda, c, b, "tiles 2^20 apart")


def test_zero_gradient_tile_next_to_a_live_one(cuda):
    """(iii) dx is exactly zero where no sample of a pixel with gradient reaches (a zero bound admits no error)."""
    from slenderobjdet_amd.layers import functional as HF

    c = _two_tile_case(502, None)
    c.dy[:, :, :8] = 0
    b = D.backward(c.x, c.R, c.w, c.dy)
    assert bool((b.dxA2 == 0).any()) and bool((b.dxA2 > 0).any())
    _run_both(HF, cuda, c, b, "zero-dY tile")


def test_nan_gradient_at_one_pixel(cuda):
    """(v) one NaN in dy: dx, d offset and d mask are non-finite exactly where the reference's are and within bounds everywhere else
    (the tile of the NaN takes the float path: ``finite_scale == false``)."""
    from slenderobjdet_amd.layers import functional as HF

    c = _two_tile_case(503, "rand")
    c.dy[0, 2, 3, 5] = float("nan")
    b = D.backward(c.x, c.R, c.w, c.dy, c.mask, c.logit)
    assert 0 < int((~torch.isfinite(b.dx)).sum()) < b.dx.numel() // 2
    assert int((~torch.isfinite(b.doff)).sum()) > 0 and int((~torch.isfinite(b.dmask)).sum()) > 0
    _run_both(HF, cuda, c, b, "NaN in dy")
    # the plain kernel on the same data (C = 64, dg 4: 16 channels per group keep it off the tiled kernel)
    c4 = D.make_case(1, 64, 128, 8, 16, dg=4, program="random", mask="rand", seed=504)
    c4.ld = None
    c4.dy[0, 2, 3, 5] = float("nan")
    b4 = D.backward(c4.x, c4.R, c4.w, c4.dy, c4.mask, c4.logit)
    d4 = _Dev(c4, cuda)
    _assert_all("NaN in dy, plain", _check_grads(c4, b4, *_col2im(HF, c4, d4, D.rb(b4.dcols.float()).to(cuda).bfloat16()), None, "bf16", "plain"))


@pytest.mark.parametrize("name", [n for n in D.BWD_CASES if D.BWD_CASES[n].get("mask") == "zero_tile"])
def test_mask_gradient_on_a_zero_mask_tile(cuda, name):
    """(iv) the mask is zero over tile (0, 0) for the last deformable group while the column gradients are not: d mask = sum_c dcols *
    sample there.  dcn_col2im_tile_kernel used to return early on max|dcols * m| == 0 and left d mask at zero."""
    from slenderobjdet_amd.layers import functional as HF

    c, _, b = _case("BWD_CASES", name)
    d = _Dev(c, cuda)
    if c.path == "fused":
        doff, dmask = d.grads()
        HF.deform_conv_bwd_fused(d.dy, d.wt, d.x, d.off, d.mask, *d.geo, doff, dmask)
    else:
        _, _, dmask = _col2im(HF, c, d, D.rb(b.dcols.float()).to(cuda).bfloat16())
    shape = (c.N, c.Ho, c.Wo, c.dg, c.taps)
    got, ref = dmask.cpu().reshape(shape)[:, :D.TILE, :D.TILE, c.dg - 1], b.dmask.reshape(shape)[:, :D.TILE, :D.TILE, c.dg - 1]
    assert float(ref.abs().max()) > 0
    print("RATIO zero-mask tile", name, "max|got| %.3g max|ref| %.3g" % (float(got.abs().max()), float(ref.abs().max())))
    r = D.check_dmask(dmask.cpu(), b, enforce=False)
    assert r["ratio"] <= 1.0, r
