"""A float64 restatement of deformable convolution v1 / v2 (forward, weight gradient, column gradient, input / offset / mask
gradients) for the operator-level tests, CPU only, and the per-element comparison the tests hold the HIP kernels
(csrc/deform_conv.hip, csrc/dcn_fused.hip) to.  No import of the product.  Written from the rule in oracle/deform_conv.py and
SURVEY.md Appendix C.11.

Layout is the kernels': x (N, H, W, C), offsets (N, Ho, Wo, >= 2 * taps * dg) fp32 with channel 2k = dy and 2k + 1 = dx of
k = g * taps + tap, tap = i * KW + j; mask (N, Ho, Wo, >= taps * dg) fp32 (values, or logits with ``logit=True``); weights
(K, taps, C); dy (N, Ho, Wo, K).  Inputs are the values the kernel sees (x, dy, w already rounded to bf16 for the bf16 paths).

Sample positions are formed as the kernels form them - ONE fp32 addition of the exact integer base ``ho * stride - pad + i * dil``
and the fp32 offset - so the floor and validity decisions are the kernel's own and no element has to be left out of any
comparison.  Everything after that addition is float64.

Every result comes with ``A``, the sum of the absolute values of its addends; dx, d offset and d mask have two: ``A1`` with
``|dcols|`` and ``A2`` with ``sum_k |dy_k| |w_k|`` in its place (dcols is itself a rounded sum of K products).  The bounds, with
``u = 2^-24`` and ``n`` the number of addends of the element:

    bf16 forward       2^-8 |ref| + (2^-9 + n u) A     output rounding; one bf16 rounding per column value; fp32 accumulation
    out_f32 forward    (2^-9 + n u) A
    column buffer      2^-8 |ref| + 8 u A               four products of three factors, one mask product
    fp32 mode          (n + 8) u A  (+ K u A2 where the column gradient is itself an fp32 sum)
    dW                 (2^-8 + n u) A                   n = pixels
    dx                 (2^-8 + n u) A1 + K u A2 + sum over contributions of quantum / 2
    d offset, d mask   (2^-8 + n u) A1 + K u A2         for logits the chain factor m (1 - m) is part of A, + 4 u A1' (below)

Two terms are wider than first proposed, each because a CORRECT kernel exceeds the narrower one (the fp32 emulation of the host
test does, by up to 1.9x):

* The rounding of a column value or column gradient to bf16 is 2^-8, not 2^-9, in dW, dx, d offset and d mask.  bf16 keeps 8
  significand bits; round-to-nearest errs by at most half a unit in the last place, 2^-9 * 2^e for 2^e <= |v| < 2^(e+1), which is
  2^-8 |v| just above a power of two and 2^-9 |v| just below the next.  An element of these gradients can have a single addend
  (dW at P = 1, a dx cell one sample reaches, d offset of a sample with one live channel vector), so the worst case is met.  The
  forward sums taps * C >= 576 rounded values; there the proposed 2^-9 stands (the emulation stays below 0.7 of the bound).
* With mask logits, d mask carries m (1 - m) with m = 1 / (1 + exp(-l)) formed in fp32: m is off by up to 2 u (the exponential,
  the sum and the quotient, of values <= 1), 1 - m inherits that ABSOLUTE error, so the product is off by up to 4 u however small
  it is (at l = +30, m rounds to 1 and the kernels' chain factor is exactly 0 where the true one is 9e-14).  The bound therefore
  adds 4 u A1', with A1' the absolute-addend sum WITHOUT the chain factor.

The quantum is that of the contributing pixel's 8x8 tile and 32-channel chunk, from the kernels' stated rule
(``fbits = 30 - ceil_log2(64 * taps)``, ``2^ex >`` the tile's magnitude bound) with ``ex + 1`` allowed: the kernel's fp32 maximum
or norm may land on the other side of a power of two.  Nothing here is tuned to what the kernels give.

tests/test_deform_conv_restated_host.py pins the restatement to oracle/deform_conv.py and its autograd, shows that an fp32
emulation with the kernels' bf16 roundings satisfies every bound, and that eight kinds of wrong answer are rejected.
"""
import math
from types import SimpleNamespace

import torch

U = 2.0 ** -24
B8 = 2.0 ** -8
B9 = 2.0 ** -9
TILE = 8          # output pixels per tile edge of the tiled / fused backward kernels
CHUNK = 32        # channels per workgroup of those kernels


def rb(t):
    """Round to bf16 and back to fp32: the storage precision of the kernels' activations, weights and column values."""
    return t.to(torch.bfloat16).to(torch.float32)


def out_size(H, W, ksize, stride, pad, dil):
    return ((H + 2 * pad - dil * (ksize[0] - 1) - 1) // stride + 1, (W + 2 * pad - dil * (ksize[1] - 1) - 1) // stride + 1)


def base_positions(Ho, Wo, ksize, stride, pad, dil):
    """Exact integer sample bases (1, Ho, 1, 1, taps) and (1, 1, Wo, 1, taps)."""
    KH, KW = ksize
    t = torch.arange(KH * KW)
    ki, kj = t // KW, t % KW
    by = (torch.arange(Ho) * stride - pad).view(1, Ho, 1, 1, 1) + (ki * dil).view(1, 1, 1, 1, -1)
    bx = (torch.arange(Wo) * stride - pad).view(1, 1, Wo, 1, 1) + (kj * dil).view(1, 1, 1, 1, -1)
    return by, bx


def restate(off, H, W, ksize, stride, pad, dil, dg):
    """Per (image, output pixel, deformable group, tap): sample position, ``valid``, the four corners' flat indices, ``ok`` flags and
    bilinear weights (corner order 00, 01, 10, 11 = (yl, xl), (yl, xh), (yh, xl), (yh, xh)).  Tensors are (N, Ho, Wo, dg, taps),
    the corner ones (4, N, Ho, Wo, dg, taps)."""
    assert off.dtype == torch.float32
    N, Ho, Wo, _ = off.shape
    taps = ksize[0] * ksize[1]
    o = off[..., :2 * taps * dg].reshape(N, Ho, Wo, dg, taps, 2)
    by, bx = base_positions(Ho, Wo, ksize, stride, pad, dil)
    py = (by.float() + o[..., 0]).double()            # the kernels' one fp32 addition
    px = (bx.float() + o[..., 1]).double()
    py64, px64 = by.double() + o[..., 0].double(), bx.double() + o[..., 1].double()
    fin = torch.isfinite(py64) & torch.isfinite(px64)
    floors_agree = bool((((py.floor() == py64.floor()) & (px.floor() == px64.floor())) | ~fin).all())
    valid = (py > -1) & (px > -1) & (py < H) & (px < W)
    fy, fx = py.floor(), px.floor()
    ly, lx = py - fy, px - fx
    hy, hx = 1 - ly, 1 - lx
    yl, xl = fy.clamp(-2, H + 1).long(), fx.clamp(-2, W + 1).long()
    idx, ok, wt = [], [], []
    for dyc, wy in ((0, hy), (1, ly)):
        for dxc, wx in ((0, hx), (1, lx)):
            yy, xx = yl + dyc, xl + dxc
            ok.append(valid & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1))
            idx.append(yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1))
            wt.append(wy * wx)
    return SimpleNamespace(py=py, px=px, valid=valid, ly=ly, lx=lx, hy=hy, hx=hx, idx=torch.stack(idx), ok=torch.stack(ok), wt=torch.stack(wt),
                           floors_agree=floors_agree, H=H, W=W, N=N, Ho=Ho, Wo=Wo, dg=dg, taps=taps, ksize=tuple(ksize), stride=stride, pad=pad, dil=dil)


def mask_values(mask, R, logit=False):
    """(N, Ho, Wo, dg, taps) float64 modulation (ones without a mask) and the chain factor dm / d(stored value)."""
    if mask is None:
        one = torch.ones(R.N, R.Ho, R.Wo, R.dg, R.taps, dtype=torch.float64)
        return one, one
    m = mask[..., :R.taps * R.dg].reshape(R.N, R.Ho, R.Wo, R.dg, R.taps).double()
    if logit:
        m = torch.sigmoid(m)
        return m, m * (1 - m)
    return m, torch.ones_like(m)


def _gather(x, R):
    """The four corner values (4, N, Ho, Wo, dg, taps, cg) float64, zero where the corner is not ``ok``."""
    N, H, W, C = x.shape
    cg = C // R.dg
    xg = x.double().reshape(N, H * W, R.dg, cg).permute(0, 2, 1, 3)                       # (N, dg, HW, cg)
    out = []
    for c in range(4):
        i = R.idx[c].permute(0, 3, 1, 2, 4).reshape(N, R.dg, -1, 1).expand(-1, -1, -1, cg)
        v = torch.gather(xg, 2, i).reshape(N, R.dg, R.Ho, R.Wo, R.taps, cg).permute(0, 2, 3, 1, 4, 5)
        out.append(torch.where(R.ok[c].unsqueeze(-1), v, torch.zeros((), dtype=torch.float64)))
    return torch.stack(out)


def _scatter(vals, R, HW):
    """Adds vals (4, N, Ho, Wo, dg, taps, cg) - already zero where not ``ok`` - at the corners' cells: (N, H, W, dg * cg)."""
    N, cg = R.N, vals.shape[-1]
    out = torch.zeros(N, R.dg, HW, cg, dtype=torch.float64)
    for c in range(4):
        i = R.idx[c].permute(0, 3, 1, 2, 4).reshape(N, R.dg, -1, 1).expand(-1, -1, -1, cg)
        out.scatter_add_(2, i, vals[c].permute(0, 3, 1, 2, 4, 5).reshape(N, R.dg, -1, cg))
    return out.permute(0, 2, 1, 3).reshape(N, R.H, R.W, R.dg * cg)


def _wg(w, R):
    K, taps, C = w.shape
    return w.double().reshape(K, taps, R.dg, C // R.dg).permute(0, 2, 1, 3)             # (K, dg, taps, cg)


def columns(x, R, mask=None, logit=False):
    """cols and the absolute-addend sum, (N, Ho, Wo, dg, taps, cg) each; also the un-masked sample and its absolute sum."""
    v = _gather(x, R)
    wt = R.wt.unsqueeze(-1)
    samp, sampA = (wt * v).sum(0), (wt * v.abs()).sum(0)
    m, _ = mask_values(mask, R, logit)
    return samp * m.unsqueeze(-1), sampA * m.abs().unsqueeze(-1), samp, sampA, v


def cols_flat(t, R):
    """(N, Ho, Wo, dg, taps, cg) -> the column buffer's (N, Ho, Wo, taps * C), channel = tap * C + g * cg + c."""
    return t.permute(0, 1, 2, 4, 3, 5).reshape(R.N, R.Ho, R.Wo, -1)


def cols_unflat(t, R):
    cg = t.shape[-1] // (R.taps * R.dg)
    return t.reshape(R.N, R.Ho, R.Wo, R.taps, R.dg, cg).permute(0, 1, 2, 4, 3, 5)


def forward(x, R, w, mask=None, logit=False, bias=None, relu=False):
    """y (N, Ho, Wo, K), its absolute-addend sum, the number of addends, and the column buffer with its sum."""
    cols, colsA, _, _, _ = columns(x, R, mask, logit)
    wg = _wg(w, R)
    y = torch.einsum("nhwgtc,kgtc->nhwk", cols, wg)
    A = torch.einsum("nhwgtc,kgtc->nhwk", colsA, wg.abs())
    n = R.taps * x.shape[-1]
    if bias is not None:
        y, A, n = y + bias.double(), A + bias.double().abs(), n + 1
    if relu:
        y = torch.relu(y)
    return SimpleNamespace(y=y, A=A, n=n, cols=cols_flat(cols, R), colsA=cols_flat(colsA, R))


def backward(x, R, w, dy, mask=None, logit=False, dcols=None, keep_pixels=None):
    """All gradients in float64.  ``dcols`` (N, Ho, Wo, taps * C) replaces dy x w (then A2 = A1 and w, dy may be None: no dW).
    ``keep_pixels`` (N, Ho, Wo) bool drops the other pixels' gradient (the host test's skipped-edge wrong answer)."""
    C = x.shape[-1]
    cols, colsA, samp, sampA, v = columns(x, R, mask, logit)
    m, chain = mask_values(mask, R, logit)
    out = SimpleNamespace(K=0, npix=R.N * R.Ho * R.Wo)
    if dcols is None:
        d = dy.double()
        if keep_pixels is not None:
            d = d * keep_pixels.unsqueeze(-1)
        wg = _wg(w, R)
        dc = torch.einsum("nhwk,kgtc->nhwgtc", d, wg)
        dcA2 = torch.einsum("nhwk,kgtc->nhwgtc", d.abs(), wg.abs())
        out.K = w.shape[0]
        out.dw = torch.einsum("nhwk,nhwgtc->kgtc", d, cols).permute(0, 2, 1, 3).reshape(w.shape)
        out.dwA = torch.einsum("nhwk,nhwgtc->kgtc", d.abs(), colsA).permute(0, 2, 1, 3).reshape(w.shape)
    else:
        dc = cols_unflat(dcols.double(), R)
        if keep_pixels is not None:
            dc = dc * keep_pixels.view(R.N, R.Ho, R.Wo, 1, 1, 1)
        dcA2 = dc.abs()
    out.dcols, out.dcolsA = cols_flat(dc, R), cols_flat(dcA2, R)
    m6, okf, wt = m.unsqueeze(-1), R.ok.unsqueeze(-1), R.wt.unsqueeze(-1)
    zero = torch.zeros((), dtype=torch.float64)
    HW = R.H * R.W
    out.dx = _scatter(torch.where(okf, wt * (dc * m6), zero), R, HW)
    out.dxA1 = _scatter(torch.where(okf, wt * (dc * m6).abs(), zero), R, HW)
    out.dxA2 = _scatter(torch.where(okf, wt * (dcA2 * m6.abs()), zero), R, HW)
    out.dxn = _scatter(okf.double(), R, HW).repeat_interleave(C // R.dg, dim=-1)         # contributions per cell (one count per group)
    hy, hx, ly, lx = (t.unsqueeze(-1) for t in (R.hy, R.hx, R.ly, R.lx))
    va = v.abs()
    gy, gx = hx * (v[2] - v[0]) + lx * (v[3] - v[1]), hy * (v[1] - v[0]) + ly * (v[3] - v[2])
    gyA, gxA = hx * (va[2] + va[0]) + lx * (va[3] + va[1]), hy * (va[1] + va[0]) + ly * (va[3] + va[2])
    val = R.valid

    def red(t):
        return torch.where(val, t.sum(-1), zero)

    def offs(a, b):
        return torch.stack([a, b], dim=-1).reshape(R.N, R.Ho, R.Wo, -1)

    out.doff = offs(red(dc * m6 * gy), red(dc * m6 * gx))
    out.doffA1 = offs(red((dc * m6).abs() * gyA), red((dc * m6).abs() * gxA))
    out.doffA2 = offs(red(dcA2 * m6.abs() * gyA), red(dcA2 * m6.abs() * gxA))
    out.doffn = x.shape[-1] // R.dg
    if mask is not None:
        out.dmask = (red(dc * samp) * chain).reshape(R.N, R.Ho, R.Wo, -1)
        out.dmaskA1 = (red(dc.abs() * sampA) * chain).reshape(R.N, R.Ho, R.Wo, -1)
        out.dmaskA2 = (red(dcA2 * sampA) * chain).reshape(R.N, R.Ho, R.Wo, -1)
        out.dmaskC = (red(dc.abs() * sampA) * (4 * U if logit else 0.0)).reshape(R.N, R.Ho, R.Wo, -1)      # the chain factor's own fp32 error
    return out


# ------------------------------------------------------------------ the fixed-point window
def fbits(taps):
    """``30 - ceil_log2(64 * taps)``: 3x3 -> 20, 1x1 -> 24, 5x5 -> 19."""
    return 30 - math.ceil(math.log2(64 * taps))


def _tile_max(t, R):
    """t (N, Ho, Wo, ...) -> max over each 8x8 tile, broadcast back to the pixels (NaN propagates)."""
    N, Ho, Wo = t.shape[:3]
    Hp, Wp = -(-Ho // TILE) * TILE, -(-Wo // TILE) * TILE
    p = torch.zeros((N, Hp, Wp) + tuple(t.shape[3:]), dtype=t.dtype)
    p[:, :Ho, :Wo] = t
    q = p.reshape((N, Hp // TILE, TILE, Wp // TILE, TILE) + tuple(t.shape[3:])).amax(dim=(2, 4), keepdim=True)
    return q.expand((N, Hp // TILE, TILE, Wp // TILE, TILE) + tuple(t.shape[3:])).reshape(p.shape)[:, :Ho, :Wo]


def _quantum_of(dmax, taps):
    """2^(ex + 1 - fbits) with 2^ex > dmax >= 2^(ex - 1) (frexp); zero where the tile takes the float path (dmax zero or not finite)."""
    live = torch.isfinite(dmax) & (dmax > 0)
    ex = torch.frexp(torch.where(live, dmax, torch.ones_like(dmax)))[1]
    return torch.where(live, torch.ldexp(torch.ones_like(dmax), ex + 1 - fbits(taps)), torch.zeros_like(dmax))


def quantum_tiled(dcols, R, mask=None, logit=False):
    """Per (pixel, channel) the quantum of the pixel's tile and the channel's 32-chunk in dcn_col2im_tile_kernel:
    ``2^ex > max |bf16(dcols) * m|`` over the tile's pixels, taps and the chunk's channels.  (N, Ho, Wo, C)."""
    m, _ = mask_values(mask, R, logit)
    dc = cols_unflat(rb(dcols.float()).double(), R) * m.unsqueeze(-1)                  # (N, Ho, Wo, dg, taps, cg)
    C = dc.shape[3] * dc.shape[5]
    a = dc.abs().amax(dim=4).reshape(R.N, R.Ho, R.Wo, C // CHUNK, CHUNK).amax(dim=-1)  # (N, Ho, Wo, chunks)
    return _quantum_of(_tile_max(a, R), R.taps).repeat_interleave(CHUNK, dim=-1)


def quantum_fused(dy, w, R, mask=None, logit=False):
    """The same for dcn_bwd_fused_kernel: ``max_p ||dY[p]|| * max ||W[:, tap, c]|| * max |m|`` over the tile / the chunk / the tile."""
    K, taps, C = w.shape
    m, _ = mask_values(mask, R, logit)
    nmax = _tile_max(dy.double().square().sum(-1).sqrt(), R)                              # (N, Ho, Wo)
    wn = w.double().square().sum(0).sqrt().amax(dim=0).reshape(C // CHUNK, CHUNK).amax(dim=-1)          # (chunks,)
    mmax = _tile_max(m.abs().amax(dim=-1), R)                                              # (N, Ho, Wo, dg)
    mmax = mmax.repeat_interleave(C // R.dg // CHUNK, dim=-1)                              # (N, Ho, Wo, chunks)
    return _quantum_of(nmax.unsqueeze(-1) * wn * mmax, taps).repeat_interleave(CHUNK, dim=-1)


def dx_quantum_sum(qpix, R):
    """Sum over the window contributions to each dx cell of half the contributing pixel's quantum (N, H, W, C)."""
    C = qpix.shape[-1]
    q = (0.5 * qpix).reshape(R.N, R.Ho, R.Wo, R.dg, 1, C // R.dg).expand(-1, -1, -1, -1, R.taps, -1)
    zero = torch.zeros((), dtype=torch.float64)
    return _scatter(torch.where(R.ok.unsqueeze(-1), q.unsqueeze(0), zero), R, R.H * R.W)


# ------------------------------------------------------------------ comparisons
def _measure(got, ref, bound, what, enforce):
    """Largest ``|got - ref| / bound`` over ALL elements.  Where the reference is not finite the result must be not finite as well (and
    the reverse); an element with a zero bound must be exact."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    fin = torch.isfinite(ref)
    same_set = bool((torch.isfinite(got) == fin).all())
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    b = torch.where(fin, bound, torch.ones_like(ref))
    ratio = torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    out = {"ratio": worst, "same_nonfinite": same_set, "compared": int(ref.numel())}
    if enforce:
        assert same_set, "%s: the non-finite elements are not the reference's" % what
        assert worst <= 1.0, "%s: |err| / bound = %.3g at %s" % (what, worst, tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0]))
    return out


def check_fwd(got, f, mode="bf16", what="dcn fwd", enforce=True):
    """mode: "bf16" (rounded output), "out_f32" (bf16 columns, fp32 output), "f32" (fp32 throughout)."""
    if mode == "bf16":
        bound = B8 * f.y.abs() + (B9 + f.n * U) * f.A
    elif mode == "out_f32":
        bound = (B9 + f.n * U) * f.A
    else:
        bound = (f.n + 8) * U * f.A
    return _measure(got, f.y, bound, what, enforce)


def check_cols(got, f, mode="bf16", what="dcn cols", enforce=True):
    bound = B8 * f.cols.abs() + 8 * U * f.colsA if mode == "bf16" else (4 + 8) * U * f.colsA
    return _measure(got, f.cols, bound, what, enforce)


def check_dw(got, b, what="dcn dW", enforce=True, scale=None):
    """``scale`` (K,): the qscale factor per output channel (exact powers of two in the tests, so the bound scales with it)."""
    ref, A = b.dw, b.dwA
    if scale is not None:
        s = scale.double().view(-1, 1, 1)
        ref, A = ref * s, A * s.abs()
    return _measure(got, ref, (B8 + b.npix * U) * A, what, enforce)


def check_dx(got, b, qsum=None, mode="bf16", what="dcn dx", enforce=True):
    if mode == "f32":
        bound = (b.dxn + 8) * U * b.dxA1 + b.K * U * b.dxA2
    else:
        bound = (B8 + b.dxn * U) * b.dxA1 + b.K * U * b.dxA2
    if qsum is not None:
        bound = bound + qsum
    return _measure(got, b.dx, bound, what, enforce)


def check_doff(got, b, mode="bf16", what="dcn d offset", enforce=True):
    got = got[..., :b.doff.shape[-1]]            # a pitched buffer's padding columns are the caller's to check
    bound = ((b.doffn + 8) * U if mode == "f32" else B8 + b.doffn * U) * b.doffA1 + b.K * U * b.doffA2
    return _measure(got, b.doff, bound, what, enforce)


def check_dmask(got, b, mode="bf16", what="dcn d mask", enforce=True):
    got = got[..., :b.dmask.shape[-1]]
    bound = ((b.doffn + 8) * U if mode == "f32" else B8 + b.doffn * U) * b.dmaskA1 + b.K * U * b.dmaskA2 + b.dmaskC
    return _measure(got, b.dmask, bound, what, enforce)


# ------------------------------------------------------------------ offset programs and cases
def border_positions(L):
    """The eleven positions per axis of the ``border`` program, all multiples of 1/8."""
    return [-1.5, -1.0, -0.875, -0.125, 0.0, L - 1.0, L - 0.875, L - 0.125, float(L), L + 0.5, float(L // 2)]


def offsets(program, N, H, W, ksize, stride, pad, dil, dg, seed, spread=4.3):
    """(N, Ho, Wo, 2 * taps * dg) fp32.

    ``random``: (rand - 0.5) * spread + 0.017, fp32.  ``border``: random (spread 1.9), then every tap of every group of the pixels
    p = 0, 1, ... in raster order samples (ys[p % 11], xs[(p // 11 + p) % 11]) of :func:`border_positions` - as many of the 121
    pairs as the map has pixels (image n starts at pair 37 n).  ``converge``: every tap of every pixel of tile (0, 0) samples
    exactly input pixel (3, 3) * stride of that tile; the other pixels are random."""
    Ho, Wo = out_size(H, W, ksize, stride, pad, dil)
    taps = ksize[0] * ksize[1]
    g = torch.Generator().manual_seed(seed)
    sp = spread if program == "random" else 1.9
    off = ((torch.rand(N, Ho, Wo, dg, taps, 2, generator=g) - 0.5) * sp + 0.017).float()
    by, bx = base_positions(Ho, Wo, ksize, stride, pad, dil)
    by, bx = by.float().expand(N, Ho, Wo, dg, taps), bx.float().expand(N, Ho, Wo, dg, taps)
    if program == "border":
        ys, xs = border_positions(H), border_positions(W)
        for n in range(N):
            for p in range(Ho * Wo):
                q = p + 37 * n
                ho, wo = divmod(p, Wo)
                off[n, ho, wo, :, :, 0] = ys[q % 11] - by[n, ho, wo]
                off[n, ho, wo, :, :, 1] = xs[(q // 11 + q) % 11] - bx[n, ho, wo]
    elif program == "converge":
        h8, w8 = min(Ho, TILE), min(Wo, TILE)
        ty, tx = min(3 * stride, H - 1), min(3 * stride, W - 1)
        off[:, :h8, :w8, :, :, 0] = ty - by[:, :h8, :w8]
        off[:, :h8, :w8, :, :, 1] = tx - bx[:, :h8, :w8]
    elif program != "random":
        raise ValueError(program)
    return off.reshape(N, Ho, Wo, 2 * taps * dg)


def masks(kind, N, Ho, Wo, taps, dg, seed):
    """``rand`` in (0, 1); ``zeros``: exact zeros at scattered pixels; ``zero_tile``: zero over tile (0, 0) for the last group;
    ``logit``: logits, randn * 3 with +-30 at scattered places (returned with logit=True).  Returns (mask or None, logit)."""
    if kind is None:
        return None, False
    g = torch.Generator().manual_seed(seed + 7)
    if kind == "logit":
        m = torch.randn(N, Ho, Wo, dg, taps, generator=g) * 3
        flat = m.view(-1)
        flat[::7] = 30.0
        flat[3::11] = -30.0
        return m.reshape(N, Ho, Wo, -1).float(), True
    m = torch.rand(N, Ho, Wo, dg, taps, generator=g) * 0.98 + 0.01
    if kind == "zeros":
        m.view(-1)[::5] = 0.0
        m[:, ::3, 1::2] = 0.0
    elif kind == "zero_tile":
        m[:, :TILE, :TILE, dg - 1] = 0.0
    elif kind != "rand":
        raise ValueError(kind)
    return m.reshape(N, Ho, Wo, -1).float(), False


def pitched(t, ld):
    """The same rows in a buffer of row pitch ``ld`` (padding columns zero)."""
    out = torch.zeros(t.shape[:-1] + (ld,), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def make_case(N, C, K, H, W, ksize=(3, 3), stride=1, pad=1, dil=1, dg=1, program="random", spread=4.3, mask=None, seed=0, f32=False, wscale=0.1):
    """One case's inputs in kernel layout: x, w, dy hold bf16 values (fp32 values with ``f32``), offsets and mask are fp32."""
    g = torch.Generator().manual_seed(seed)
    r = (lambda t: t) if f32 else rb
    Ho, Wo = out_size(H, W, ksize, stride, pad, dil)
    taps = ksize[0] * ksize[1]
    x = r(torch.randn(N, H, W, C, generator=g))
    w = r(torch.randn(K, taps, C, generator=g) * wscale)
    dy = r(torch.randn(N, Ho, Wo, K, generator=g))
    bias = torch.randn(K, generator=g)
    off = offsets(program, N, H, W, ksize, stride, pad, dil, dg, seed + 1, spread)
    m, logit = masks(mask, N, Ho, Wo, taps, dg, seed)
    R = restate(off, H, W, ksize, stride, pad, dil, dg)
    return SimpleNamespace(x=x, w=w, dy=dy, bias=bias, off=off, mask=m, logit=logit, R=R, N=N, C=C, K=K, H=H, W=W, Ho=Ho, Wo=Wo, ksize=tuple(ksize),
                           stride=stride, pad=pad, dil=dil, dg=dg, taps=taps, f32=f32)


# ------------------------------------------------------------------ the case tables (shared by the host and the device tests)
def _c(N, C, K, H, W, **kw):
    return dict(N=N, C=C, K=K, H=H, W=W, **kw)


# forward: "paths" names what the device test runs: cols (deform_im2col), gemm (+ conv2d_fwd, bf16 and out_f32), fused, f32
FWD_CASES = {
    "base_border": _c(2, 128, 72, 9, 11, program="border", mask="rand"),
    "base_random": _c(2, 128, 72, 9, 11, program="random"),
    "q2_k264_dg2_s2": _c(1, 256, 264, 13, 10, dg=2, stride=2, program="border", mask="zeros"),       # second q tile, of 8 channels
    "p128_1x1": _c(1, 128, 128, 8, 16, ksize=(1, 1), pad=0, program="border", mask="rand"),         # P = 128 exactly
    "p129": _c(1, 128, 128, 3, 43, program="random", mask="zero_tile"),                             # P = 129
    "p1": _c(1, 128, 8, 1, 1, program="random", spread=1.9, mask="rand"),                           # P = 1
    "dil2": _c(2, 128, 64, 9, 11, dil=2, pad=2, program="border"),
    "pad0": _c(2, 128, 64, 9, 11, pad=0, program="border", mask="rand"),
    "k5_cols": _c(1, 64, 32, 7, 7, ksize=(5, 5), pad=2, program="border", mask="rand", paths=("cols", "gemm")),
    "pitched_logit": _c(2, 128, 72, 9, 11, program="border", mask="logit", ld=32),
    "f32_c16": _c(2, 16, 12, 9, 11, program="border", mask="rand", f32=True, paths=("f32",)),
    "f32_c24_dg3": _c(1, 24, 12, 9, 11, dg=3, stride=2, program="random", mask="logit", f32=True, paths=("f32",)),
}

# weight gradient: C in {64, 128, 256 with dg 2} x K in {8, 264} x P in {1, 63, 64, 65}, with and without qscale
WGRAD_CASES = {
    "c64_k8_p1": _c(1, 64, 8, 1, 1, program="random", spread=1.9, mask="rand"),
    "c64_k264_p63_q": _c(1, 64, 264, 7, 9, program="border", qscale=True),
    "c128_k8_p64_q": _c(1, 128, 8, 8, 8, program="random", mask="zeros", qscale=True),
    "c128_k264_p65": _c(1, 128, 264, 5, 13, program="border", mask="rand"),
    "c256_dg2_k264_p63_q": _c(1, 256, 264, 7, 9, dg=2, program="border", mask="logit", qscale=True),
    "c256_dg2_k8_p65": _c(1, 256, 8, 13, 5, dg=2, program="random"),
}

# input / offset / mask gradients.  path: plain (dcn_col2im_kernel<bf16>), tiled (dcn_col2im_tile_kernel), f32 (dcn_col2im_kernel<float>),
# fused (dcn_bwd_fused_kernel, run at 2 and 4 px of window slack)
BWD_CASES = {
    "plain_c64_dg4": _c(2, 64, 32, 9, 11, dg=4, program="border", mask="rand", path="plain"),                   # red = 2: shuffles
    "plain_c48_red0": _c(2, 48, 32, 9, 11, program="border", mask="rand", path="plain", ld=24),                        # red = 0: float atomics
    "plain_c96_dg2_red0": _c(1, 96, 32, 9, 11, dg=2, program="random", mask="zero_tile", path="plain"),
    "plain_c64_s2": _c(1, 64, 32, 17, 9, stride=2, program="border", path="plain"),                             # 3x3 stride 2: no window fits
    "tiled_c64": _c(2, 64, 32, 9, 11, program="border", mask="rand", path="tiled"),
    "tiled_c64_dg2_zero_tile": _c(1, 64, 32, 9, 11, dg=2, program="random", mask="zero_tile", path="tiled"),
    "tiled_c64_dg2_spread14": _c(1, 64, 32, 17, 9, dg=2, program="random", spread=14.0, mask="zeros", path="tiled"),
    "tiled_1x1": _c(1, 64, 32, 9, 11, ksize=(1, 1), pad=0, program="border", mask="logit", path="tiled", ld=32),
    "tiled_1x1_s2": _c(1, 64, 32, 17, 9, ksize=(1, 1), pad=0, stride=2, program="border", path="tiled"),
    "tiled_5x5": _c(1, 64, 32, 9, 11, ksize=(5, 5), pad=2, program="random", mask="rand", path="tiled"),
    "tiled_converge": _c(1, 64, 32, 9, 11, program="converge", mask="rand", path="tiled"),
    "f32_c16": _c(2, 16, 12, 9, 11, program="border", mask="rand", f32=True, path="f32"),                       # red = 2
    "f32_c48_red0": _c(1, 48, 12, 9, 11, program="random", mask="logit", f32=True, path="f32"),
    "fused_c32_k128_8x8": _c(1, 32, 128, 8, 8, program="converge", path="fused"),
    "fused_c64_k256_9x11": _c(2, 64, 256, 9, 11, program="border", mask="rand", path="fused", ld=32),
    "fused_c256_dg2_k512_17x9": _c(1, 256, 512, 17, 9, dg=2, program="random", mask="zero_tile", path="fused", wscale=0.05),
    "fused_c64_k128_spread14": _c(1, 64, 128, 17, 9, program="random", spread=14.0, path="fused"),
    "fused_c32_k128_5x5_logit": _c(1, 32, 128, 9, 11, ksize=(5, 5), pad=2, program="random", mask="logit", path="fused"),
    "fused_c64_k256_s2": _c(1, 64, 256, 16, 16, stride=2, program="border", mask="zeros", path="fused"),
    "fused_c64_k512_border": _c(1, 64, 512, 9, 11, program="border", path="fused", wscale=0.05),
}
_EXTRA = ("paths", "path", "ld", "qscale")


def case(table, name):
    """The inputs of a named case (seeded by its position in the table) with the table's extra fields attached."""
    spec = dict(table[name])
    extra = {k: spec.pop(k) for k in _EXTRA if k in spec}
    c = make_case(seed=1000 + 17 * list(table).index(name), **spec)
    for k in _EXTRA:
        setattr(c, k, extra.get(k))
    return c
