"""A float64 restatement of the plain convolutions (forward, data gradient, weight gradient, with the epilogue operands of the
implicit-GEMM kernels) for the operator-level tests, CPU only, and the per-element comparison the tests hold the HIP kernels
(csrc/conv_igemm.hip, conv_igemm256.hip, conv_pw.hip, conv_ws3.hip, the weight-gradient kernels, conv_dispatch.hip) to.  No import
of the product.  Written from the rule oracle/nn.py states with F.conv2d (cross-correlation, zero padding, output size
``(H + 2 pad - dil (R - 1) - 1) // stride + 1``) as one matrix product per tap; tests/test_conv_restated_host.py pins it to
oracle/nn.py and to F.conv2d(groups=) with its autograd.

Layout is the kernels': x (N, H, W, C), w (K, R, S, C / groups), dy (N, Ho, Wo, K), dw like w.  Inputs are the values the kernel sees
(x, w, dy, residual, accumulate operand and mask already bf16-representable; bias and qscale fp32).

Every result comes with ``A``, the sum of the absolute values of the element's addends (the same convolution on ``|.|`` operands, the
bias / residual / accumulate operand included), and ``n``, the number of addends (taps x contraction channels, + 1 per epilogue
operand; for dW the pixels, + 1 with ``qscale``).  The bounds, with ``u = 2^-23``:

    fp32 output, dW    acc = n u A
    bf16 output        acc + half_ulp_bf16(|ref| + acc),   half_ulp_bf16(v) = 2^(floor(log2 v) - 8)

* bf16 x bf16 products are exact in fp32 (16 significant bits).  A sum of n addends takes n - 1 additions however it is bracketed
  (K loop, matrix unit, split partial sums, atomics), and one fp32 addition errs by at most one unit in the last place of its result,
  ``u |partial sum| <= u A``, whatever the rounding direction: a matrix unit that truncates internally is covered, nearest is not
  assumed.  The n-th unit pays for the second-order terms ((1 + u)^n - 1 - n u < u for every n used here).
* The bf16 store is ONE round-to-nearest of a value t within ``acc`` of the reference: ``|t| <= |ref| + acc``, and the rounding errs by
  half a unit in the last place of t's binade.  The ulp-exact form is used, not ``2^-8 |ref|``: the relative form is up to twice as
  wide just below a power of two, and a truncating store hides there.
* ReLU is 1-Lipschitz and ``relu(t)`` is within ``acc`` of ``relu(ref)``, so the bound holds through it with ``|relu(ref)|`` in place of
  ``|ref|``.
* The ReLU mask of the data gradient is ``mask > 0`` on the given tensor (or bits), which is exact: a masked element has A = 0 and
  must be exactly zero.  No element is ever left out.
* ``qscale`` factors are exact powers of two in the tests, so reference and bound scale exactly.  A weight gradient accumulated a
  second time into its own result is compared as ``dw / 2``: two sums of n - 1 additions each, halved, and the one addition that joins
  them, ``(n - 1) u A + u |ref| <= n u A``.

Nothing here is tuned to what the kernels give.  The inputs have dynamic range: output channels are scaled by exact powers of two over
2^-6 .. 2^6 (period 13 in the channel index), contraction channels over 2^-3 .. 2^3 (period 7), so that a mistake confined to a small
channel is as visible as one in a large channel; one case per table is iid.  ReLU masks are ``relu(randn)`` rounded to bf16 - exact
zeros in half of the entries - with some entries set to ``-0.0``.
"""
import zlib
from types import SimpleNamespace

import torch

U = 2.0 ** -23


def rb(t):
    """Round to bf16 and back to fp32: the storage precision of activations and weights."""
    return t.to(torch.bfloat16).to(torch.float32)


def out_size(H, W, R, S, stride, pad, dil):
    return (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (S - 1) - 1) // stride + 1


def dense_weight(w, groups):
    """(K, R, S, C / groups) -> the block-diagonal (K, R, S, C): structural zeros add nothing to a sum or to A."""
    if groups == 1:
        return w
    K, R, S, Cg = w.shape
    Kg = K // groups
    d = w.new_zeros(K, R, S, Cg * groups)
    for g in range(groups):
        d[g * Kg:(g + 1) * Kg, :, :, g * Cg:(g + 1) * Cg] = w[g * Kg:(g + 1) * Kg]
    return d


def diagonal_blocks(dw, groups):
    """The inverse selection: dense (K, R, S, C) -> (K, R, S, C / groups)."""
    if groups == 1:
        return dw
    K, R, S, C = dw.shape
    Kg, Cg = K // groups, C // groups
    return torch.cat([dw[g * Kg:(g + 1) * Kg, :, :, g * Cg:(g + 1) * Cg] for g in range(groups)], 0)


def _window(t, r, s, Ho, Wo, stride, dil):
    """The padded tensor's pixels that tap (r, s) pairs with the output pixels: (N, Ho, Wo, C) view."""
    return t[:, r * dil:r * dil + (Ho - 1) * stride + 1:stride, s * dil:s * dil + (Wo - 1) * stride + 1:stride]


def _padded(x, pad):
    N, H, W, C = x.shape
    p = x.new_zeros(N, H + 2 * pad, W + 2 * pad, C)
    p[:, pad:pad + H, pad:pad + W] = x
    return p


def _conv(x, w, stride, pad, dil):
    N, H, W, C = x.shape
    K, R, S, _ = w.shape
    Ho, Wo = out_size(H, W, R, S, stride, pad, dil)
    xp = _padded(x, pad)
    y = x.new_zeros(N * Ho * Wo, K)
    for r in range(R):
        for s in range(S):
            y += _window(xp, r, s, Ho, Wo, stride, dil).reshape(-1, C) @ w[:, r, s].t()
    return y.reshape(N, Ho, Wo, K)


def _conv_t(dy, w, hw, stride, pad, dil):
    N, Ho, Wo, K = dy.shape
    _, R, S, C = w.shape
    H, W = hw
    assert (Ho, Wo) == out_size(H, W, R, S, stride, pad, dil)
    dxp = dy.new_zeros(N, H + 2 * pad, W + 2 * pad, C)
    d2 = dy.reshape(-1, K)
    for r in range(R):
        for s in range(S):
            _window(dxp, r, s, Ho, Wo, stride, dil).add_((d2 @ w[:, r, s]).reshape(N, Ho, Wo, C))      # distinct cells within one tap
    return dxp[:, pad:pad + H, pad:pad + W].contiguous()


def _conv_w(dy, x, R, S, stride, pad, dil):
    N, Ho, Wo, K = dy.shape
    C = x.shape[-1]
    xp = _padded(x, pad)
    d2t = dy.reshape(-1, K).t().contiguous()
    dw = dy.new_zeros(K, R, S, C)
    for r in range(R):
        for s in range(S):
            dw[:, r, s] = d2t @ _window(xp, r, s, Ho, Wo, stride, dil).reshape(-1, C)
    return dw


def up2(t):
    """Nearest 2x up-sampling of (N, h, w, C): output pixel (H, W) reads (H // 2, W // 2)."""
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def zero_stuffed(t):
    """(N, h, w, C) -> (N, 2h, 2w, C) with t at the even (H, W) and zeros elsewhere: the compact gradient of a stride-2 1x1 consumer."""
    N, h, w, C = t.shape
    z = t.new_zeros(N, 2 * h, 2 * w, C)
    z[:, ::2, ::2] = t
    return z


def forward(x, w, bias=None, res=None, res_up2=False, relu=False, *, stride=1, pad=0, dil=1, groups=1):
    """y (N, Ho, Wo, K) float64 (after the ReLU), A, n."""
    x, wd = x.double(), dense_weight(w.double(), groups)
    y, A = _conv(x, wd, stride, pad, dil), _conv(x.abs(), wd.abs(), stride, pad, dil)
    n = w.shape[1] * w.shape[2] * w.shape[3]
    if bias is not None:
        y, A, n = y + bias.double(), A + bias.double().abs(), n + 1
    if res is not None:
        r = up2(res.double()) if res_up2 else res.double()
        y, A, n = y + r, A + r.abs(), n + 1
    return (torch.relu(y) if relu else y), A, n


def dgrad(dy, w, hw, *, stride=1, pad=0, dil=1, accum=None, accum_even=False, mask=None, groups=1):
    """dx (N, H, W, C) float64 of y = conv(x, w) with w (K, R, S, C / groups): ``mask > 0 ? dx + accum : 0``, A, n."""
    dy, wd = dy.double(), dense_weight(w.double(), groups)
    dx, A = _conv_t(dy, wd, hw, stride, pad, dil), _conv_t(dy.abs(), wd.abs(), hw, stride, pad, dil)
    n = w.shape[1] * w.shape[2] * (w.shape[0] // groups)
    if accum is not None:
        a = zero_stuffed(accum.double()) if accum_even else accum.double()
        dx, A, n = dx + a, A + a.abs(), n + 1
    if mask is not None:
        keep = (mask > 0).to(torch.float64)
        dx, A = dx * keep, A * keep
    return dx, A, n


def wgrad(dy, x, R, S, *, stride=1, pad=0, dil=1, qscale=None, groups=1):
    """dw (K, R, S, C / groups) float64 of ONE level, A, n; the caller sums levels (dw, A and n all add)."""
    dy, x = dy.double(), x.double()
    dw, A = _conv_w(dy, x, R, S, stride, pad, dil), _conv_w(dy.abs(), x.abs(), R, S, stride, pad, dil)
    dw, A = diagonal_blocks(dw, groups), diagonal_blocks(A, groups)
    n = dy.shape[0] * dy.shape[1] * dy.shape[2]
    if qscale is not None:
        q = qscale.double().view(-1, 1, 1, 1)
        dw, A, n = dw * q, A * q.abs(), n + 1
    return dw, A, n


# ------------------------------------------------------------------ bounds and the comparison
def half_ulp_bf16(v):
    """2^(floor(log2 v) - 8) for v > 0, 0 for v == 0: half a unit in the last place of the bf16 binade that holds v."""
    e = torch.frexp(torch.where(v > 0, v, torch.ones_like(v)))[1]          # v = m 2^e, 0.5 <= m < 1: floor(log2 v) = e - 1
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), e - 9), torch.zeros_like(v))


def bound_f32(A, n):
    return n * U * A


def bound_bf16(ref, A, n):
    acc = n * U * A
    return acc + half_ulp_bf16(ref.abs() + acc)


def _measure(got, ref, bound, what, enforce):
    """Largest ``|got - ref| / bound`` over ALL elements.  Where the reference is not finite the result must be not finite as well (and
    the reverse); an element with a zero bound must be exact."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    fin = torch.isfinite(ref)
    same_set = bool((torch.isfinite(got) == fin).all())
    err = torch.where(fin & torch.isfinite(got), (got - ref).abs(), torch.zeros_like(ref))
    b = torch.where(fin, bound, torch.ones_like(ref))
    ratio = torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    out = {"ratio": worst, "same_nonfinite": same_set, "compared": int(ref.numel())}
    if enforce:
        assert same_set, "%s: the non-finite elements are not the reference's" % what
        assert worst <= 1.0, "%s: |err| / bound = %.3g at %s" % (what, worst, tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0]))
    return out


def check(got, ref, A, n, bf16, what="conv", enforce=True):
    """``ref, A, n`` as :func:`forward`, :func:`dgrad` or :func:`wgrad` return them; ``bf16``: the output was stored as bf16."""
    return _measure(got, ref, bound_bf16(ref, A, n) if bf16 else bound_f32(A, n), what, enforce)


def over(got, ref, A, n, bf16):
    """Share of the elements over their bound (the host test's figures)."""
    b = bound_bf16(ref, A, n) if bf16 else bound_f32(A, n)
    return float(((got.double() - ref).abs() > b).double().mean())


def current_criterion(got, ref, rel):
    """What tests/test_gpu_conv.py asks: ``max |err| / (rel max |ref|)`` - one number per tensor (<= 1 passes)."""
    return float((got.double() - ref).abs().max() / (rel * max(float(ref.abs().max()), 1e-6)))


def bits_pack(b):
    """bool (..., 8 m) -> uint8, little-endian per 8 consecutive elements, as sod_conv2d_fwd_bits stores them."""
    return (b.reshape(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


def bits_unpack(bits, shape):
    return ((bits.reshape(-1, 1).to(torch.int32) >> torch.arange(8, dtype=torch.int32)) & 1).reshape(shape).bool()


# ------------------------------------------------------------------ guarded buffers (the device test)
GUARD_BYTES = 4096
_SENTINEL = 0xA5


def guarded(shape, dtype, device, fill=None):
    """A tensor of ``shape`` inside a larger allocation with at least GUARD_BYTES of sentinel bytes before and after (the payload
    starts 4096-byte aligned).  Returns (tensor, arena); :func:`assert_guards_intact` compares the surrounding bytes bitwise."""
    numel = 1
    for s in shape:
        numel *= int(s)
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    arena = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES + 16,), _SENTINEL, dtype=torch.uint8, device=device)
    t = arena[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype).view(shape)
    if fill is not None:
        t.fill_(fill)
    return t, (arena, nbytes)


def assert_guards_intact(guard, what="output"):
    arena, nbytes = guard
    a = arena.cpu()
    assert bool((a[:GUARD_BYTES] == _SENTINEL).all()), "%s: bytes BEFORE the buffer were written" % what
    assert bool((a[GUARD_BYTES + nbytes:] == _SENTINEL).all()), "%s: bytes BEHIND the buffer were written" % what


def in_nan_arena(t, device, dtype=torch.bfloat16):
    """A copy of ``t`` on the device between at least 4 KB of NaN on either side: an out-of-range read that enters a sum shows as a
    non-finite output."""
    pad = GUARD_BYTES // 2
    arena = torch.full((pad + t.numel() + pad,), float("nan"), dtype=dtype, device=device)
    v = arena[pad:pad + t.numel()].view(t.shape)
    v.copy_(t.to(device))
    return v


# ------------------------------------------------------------------ inputs
def _gen(name, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(name.encode()) + salt) & 0x7FFFFFFF)


def out_scale(n, wide=True):
    """Per output channel: 2^-6 .. 2^6, period 13."""
    return 2.0 ** ((torch.arange(n) % 13) - 6).float() if wide else torch.ones(n)


def red_scale(n, wide=True):
    """Per contraction channel: 2^-3 .. 2^3, period 7."""
    return 2.0 ** ((torch.arange(n) % 7) - 3).float() if wide else torch.ones(n)


def relu_tensor(shape, g):
    """relu(randn) as bf16 values: exact zeros in half of the entries, every 11th entry -0.0."""
    t = rb(torch.relu(torch.randn(shape, generator=g)))
    t.view(-1)[::11] = -0.0
    return t


def fwd_inputs(name, table=None):
    """x, w, bias, res (full resolution), res_half of a forward case."""
    c = SimpleNamespace(**(table or FWD_CASES)[name])
    g = _gen(name)
    N, H, W = c.shape
    Cg = c.C // c.groups
    Ho, Wo = out_size(H, W, c.R, c.R, c.stride, c.pad, c.dil)
    so, sr = out_scale(c.K, c.wide), red_scale(c.C, c.wide)
    x = rb(torch.randn(N, H, W, c.C, generator=g)) * sr
    if c.relu_in:
        x = torch.relu(x)
        x.view(-1)[::11] = -0.0
    w = rb(torch.randn(c.K, c.R, c.R, Cg, generator=g) * (c.R * c.R * Cg) ** -0.5) * so.view(-1, 1, 1, 1)
    bias = torch.randn(c.K, generator=g) * so
    res = rb(torch.randn(N, Ho, Wo, c.K, generator=g)) * so
    res_half = rb(torch.randn(N, Ho // 2, Wo // 2, c.K, generator=g)) * so if Ho % 2 == 0 and Wo % 2 == 0 else None
    return SimpleNamespace(x=x, w=w, bias=bias, res=res, res_half=res_half, Ho=Ho, Wo=Wo, N=N, H=H, W=W, geo=dict(stride=c.stride, pad=c.pad, dil=c.dil),
                           **{k: getattr(c, k) for k in ("C", "K", "R", "groups", "variant", "knobs", "forms", "stride", "pad", "dil")})


def dgrad_inputs(name, table=None):
    """dy (N, Ho, Wo, K), w (K, R, R, C / groups), accum, mask (N, H, W, C) and accum_half (N, H / 2, W / 2, C) of a data-gradient case."""
    c = SimpleNamespace(**(table or DGRAD_CASES)[name])
    g = _gen(name, 1)
    N, H, W = c.shape
    Cg = c.C // c.groups
    Ho, Wo = out_size(H, W, c.R, c.R, c.stride, c.pad, c.dil)
    so, sr = out_scale(c.C, c.wide), red_scale(c.K, c.wide)
    dy = rb(torch.randn(N, Ho, Wo, c.K, generator=g)) * sr
    w = rb(torch.randn(c.K, c.R, c.R, Cg, generator=g) * (c.R * c.R * (c.K // c.groups)) ** -0.5)
    w = w * so.view(c.groups, 1, Cg).expand(c.groups, c.K // c.groups, Cg).reshape(c.K, 1, 1, Cg)      # column j of group g is dx channel g Cg + j
    accum = rb(torch.randn(N, H, W, c.C, generator=g)) * so
    mask = relu_tensor((N, H, W, c.C), g)
    accum_half = rb(torch.randn(N, H // 2, W // 2, c.C, generator=g)) * so if H % 2 == 0 and W % 2 == 0 else None
    return SimpleNamespace(dy=dy, w=w, accum=accum, mask=mask, accum_half=accum_half, Ho=Ho, Wo=Wo, N=N, H=H, W=W, geo=dict(stride=c.stride, pad=c.pad, dil=c.dil),
                           **{k: getattr(c, k) for k in ("C", "K", "R", "groups", "variant", "knobs", "forms", "stride", "pad", "dil")})


def wgrad_inputs(name, table=None):
    """Per level dy (N, Ho, Wo, K) and x (N, H, W, C); qscale: exact powers of two per output channel."""
    c = SimpleNamespace(**(table or WGRAD_CASES)[name])
    g = _gen(name, 2)
    so, sr = out_scale(c.K, c.wide), red_scale(c.C, c.wide)
    xs, dys = [], []
    for (H, W) in c.levels:
        Ho, Wo = out_size(H, W, c.R, c.R, c.stride, c.pad, c.dil)
        xs.append(rb(torch.randn(c.N, H, W, c.C, generator=g)) * sr)
        dys.append(rb(torch.randn(c.N, Ho, Wo, c.K, generator=g)) * so)
    qscale = 2.0 ** ((torch.arange(c.K) % 5) - 2).float()
    return SimpleNamespace(xs=xs, dys=dys, qscale=qscale, geo=dict(stride=c.stride, pad=c.pad, dil=c.dil),
                           **{k: getattr(c, k) for k in ("N", "C", "K", "R", "levels", "kernel", "groups", "stride", "pad", "dil")})


def wgrad_reference(c, qscale=False):
    """dw, A, n summed over the case's levels."""
    tot = None
    for dy, x in zip(c.dys, c.xs):
        r = wgrad(dy, x, c.R, c.R, qscale=c.qscale if qscale else None, groups=c.groups, **c.geo)
        tot = r if tot is None else (tot[0] + r[0], tot[1] + r[1], tot[2] + r[2] - (1 if qscale else 0))
    return tot


# ------------------------------------------------------------------ the case tables (shared by the host and the device tests)
# Kernel variant codes (sod_conv_last_variant): BQ * 100000 + BP * 100 + BK (+ 1 on the per-chunk gather path); 256 = conv_igemm256.hip,
# 7001 = conv_pw.hip, 7003 = conv_ws3.hip.  ``knobs``: C-ABI setter -> value while the case runs (restored to -1 / 0 afterwards).
L128, G128, K32, T64K32, T64G, T16, T16G, V256, PW, WS3 = 12812864, 12812865, 12812832, 6425632, 6425665, 1625664, 1625665, 256, 7001, 7003
FWD_ALL = ("plain", "bias_relu", "bias_res_relu", "out_f32")
DG_ALL = ("plain", "accum", "mask", "accum_mask")
T256 = {"sod_conv_set_tile256": 2}
FWS3 = {"sod_conv_set_ws3": 2}


def _f(shape, C, K, R=3, stride=1, pad=None, dil=1, variant=L128, knobs=None, forms=None, groups=1, wide=True, relu_in=False):
    return dict(shape=shape, C=C, K=K, R=R, stride=stride, pad=(R // 2) * dil if pad is None else pad, dil=dil, variant=variant, knobs=knobs or {},
                forms=forms, groups=groups, wide=wide, relu_in=relu_in)


FWD_CASES = {
    # 128x128 linear
    "l128_3x3_iid": _f((2, 13, 21), 64, 128, wide=False),
    "l128_3x3": _f((2, 13, 21), 64, 128),
    "l128_p1_1x1": _f((1, 1, 1), 64, 128, R=1),
    "l128_p128_k136": _f((1, 8, 16), 64, 136),                      # P = 128 exactly, 8 channels in the second q-tile
    "l128_p129_k136": _f((1, 3, 43), 64, 136),                      # P = 129
    "l128_s2_c128": _f((2, 14, 18), 128, 128, stride=2),            # the stride keeps it off conv_ws3 with SOD_CONV_WS3 untouched
    "l128_dil2": _f((1, 10, 10), 64, 128, dil=2),
    # 128x128 gather
    "g128_c80_k256": _f((1, 12, 10), 80, 256, variant=G128),
    # 128x128 BK = 32: grids above 512 workgroups (65 pixel tiles x 8 q-tiles = 520); P < 16384 keeps the 128-channel one off conv_pw
    "k32_1x1_c64": _f((1, 65, 127), 64, 1024, R=1, variant=K32),    # 2 K-steps
    "k32_1x1_c128": _f((1, 65, 127), 128, 1024, R=1, variant=K32),  # 4 K-steps
    "k32_3x3_c64": _f((1, 65, 127), 64, 1024, variant=K32),
    # 64x256
    "t64_s2": _f((2, 14, 18), 64, 64, stride=2, variant=T64K32),
    "t64_stem": _f((1, 18, 22), 8, 64, R=7, stride=2, variant=T64G),
    # 16x256
    "t16_c256_k8": _f((2, 11, 13), 256, 8, variant=T16),
    "t16_k5": _f((1, 7, 9), 64, 5, variant=T16),                    # Nout % 4 != 0: scalar epilogue
    "t16_c80_k8": _f((2, 11, 13), 80, 8, variant=T16G),
    # 256x256 forced
    "v256_k256": _f((2, 13, 21), 64, 256, variant=V256, knobs=T256),
    "v256_k72_1x1": _f((1, 6, 7), 64, 72, R=1, variant=V256, knobs=T256),          # a single K-step
    "v256_k720": _f((2, 13, 21), 64, 720, variant=V256, knobs=T256),
    "v256_5x5": _f((1, 12, 10), 128, 256, R=5, variant=V256, knobs=T256),
    # conv_ws3 forced: bias / ReLU only
    "ws3_one_tile": _f((1, 8, 14), 128, 128, variant=WS3, knobs=FWS3, forms=("plain", "bias_relu"), relu_in=True),
    "ws3_one_past": _f((1, 9, 15), 128, 128, variant=WS3, knobs=FWS3, forms=("plain", "bias_relu")),
    "ws3_3img": _f((3, 13, 21), 128, 128, variant=WS3, knobs=FWS3, forms=("plain", "bias_relu")),
    # conv_pw: bf16 output only
    "pw_128_512": _f((1, 129, 131), 128, 512, R=1, variant=PW, forms=("plain", "bits"), relu_in=True),
    "pw_512_128": _f((1, 129, 131), 512, 128, R=1, variant=PW, forms=("plain", "bits")),
    "pw_128_512_reverse": _f((1, 129, 131), 128, 512, R=1, variant=PW, knobs={"sod_conv_set_reverse": 1}, forms=("plain", "bits")),
    # channel window (grouped): bias + ReLU, against groups= in float64
    "cwin_s1": _f((2, 9, 11), 256, 256, groups=32, forms=("bias_relu",), relu_in=True),
    "cwin_s2": _f((2, 14, 18), 256, 256, stride=2, groups=32, forms=("bias_relu",), relu_in=True),
    # epilogue forms of their own
    "up2_1x1": _f((2, 12, 20), 64, 128, R=1, forms=("up2", "up2_f32")),
    "bits_1x1": _f((2, 19, 27), 128, 512, R=1, forms=("bits",)),
}


def _d(shape, C, K, R=3, stride=1, pad=None, dil=1, variant=L128, knobs=None, forms=None, groups=1, wide=True):
    """Data gradient of the convolution C -> K on an input of ``shape``: contracts over taps x K, stores C channels."""
    return dict(shape=shape, C=C, K=K, R=R, stride=stride, pad=(R // 2) * dil if pad is None else pad, dil=dil, variant=variant, knobs=knobs or {},
                forms=forms, groups=groups, wide=wide)


DGRAD_CASES = {
    "l128_3x3_iid": _d((2, 13, 21), 128, 64, wide=False),
    "l128_3x3": _d((2, 13, 21), 128, 64),
    "l128_s2_odd": _d((2, 15, 13), 128, 64, stride=2),              # odd input at stride 2
    "l128_dil2": _d((1, 10, 10), 128, 64, dil=2),
    "t64_s2_odd": _d((2, 15, 13), 64, 128, stride=2, variant=T64K32),      # dx of 64 channels is a 64x256 tile
    "g128_k80": _d((2, 11, 13), 256, 80, variant=G128),             # dY of 80 channels: per-chunk gather
    "g128_k72": _d((2, 11, 13), 256, 72, variant=G128),
    "k32_1x1_k64": _d((1, 65, 127), 1024, 64, R=1, variant=K32, forms=("plain", "accum_bits")),
    "k32_1x1_k128": _d((1, 65, 127), 1024, 128, R=1, variant=K32, forms=("plain", "accum_bits")),
    "t16_stem": _d((1, 18, 22), 8, 64, R=7, stride=2, variant=T16),
    "v256_k256": _d((2, 13, 21), 64, 256, variant=V256, knobs=T256),
    "v256_c256": _d((2, 13, 21), 256, 64, variant=V256, knobs=T256),
    "v256_5x5": _d((1, 12, 10), 128, 256, R=5, variant=V256, knobs=T256),
    "ws3_one_tile": _d((1, 8, 14), 128, 128, variant=WS3, knobs=FWS3, forms=("plain", "mask")),
    "ws3_one_past": _d((1, 9, 15), 128, 128, variant=WS3, knobs=FWS3, forms=("plain", "mask")),
    "ws3_3img": _d((3, 13, 21), 128, 128, variant=WS3, knobs=FWS3, forms=("plain", "mask")),
    "pw_dy128_dx512": _d((1, 129, 131), 512, 128, R=1, variant=PW, forms=("plain", "accum_bits", "mask")),
    "pw_dy512_dx128": _d((1, 129, 131), 128, 512, R=1, variant=PW, forms=("plain", "accum_bits", "mask")),
    "pw_dy128_dx512_reverse": _d((1, 129, 131), 512, 128, R=1, variant=PW, knobs={"sod_conv_set_reverse": 1}, forms=("accum_bits",)),
    "cwin_s1": _d((2, 9, 11), 256, 256, groups=32, forms=("mask",)),
    "cwin_s2": _d((2, 14, 18), 256, 256, stride=2, groups=32, forms=("mask",)),
    # bf16 accum_even (F_RES_EVEN): mask bits * (dx + accum zero-stuffed to the even pixels)
    "even_1x1": _d((2, 14, 18), 64, 128, R=1, variant=T64K32, forms=("accum_even",)),
    "even_3x3": _d((2, 14, 18), 256, 64, forms=("accum_even",)),
}


def _w(N, levels, C, K, R=3, stride=1, pad=None, dil=1, kernel="w128", groups=1, wide=True):
    return dict(N=N, levels=[tuple(l) for l in levels], C=C, K=K, R=R, stride=stride, pad=(R // 2) * dil if pad is None else pad, dil=dil, kernel=kernel,
                groups=groups, wide=wide)


# kernel: w128 = conv_wgrad_kernel (32003) at explicit splits 1 and 3 AND the ring variants 2300 / 2310; w256 = conv_wgrad256 (splits -1, 256);
# w9 = conv_wgrad9 (splits -2, 9009); fold = conv_wgrad_fold (32004), dY in the concatenated buffer; diag = the channel window's diagonal tiles
WGRAD_CASES = {
    "w128_wide_row_iid": _w(1, [(5, 70)], 64, 64, wide=False),
    "w128_wide_row": _w(1, [(5, 70)], 64, 64),
    "w128_p128_wraps": _w(3, [(2, 64)], 64, 128),
    "w128_s2": _w(2, [(14, 18)], 64, 64, stride=2),
    "w128_dil2": _w(1, [(10, 10)], 64, 64, dil=2),
    "w128_c136_k72": _w(2, [(7, 9)], 136, 72),
    "ring_3lev": _w(2, [(20, 68), (10, 34), (5, 17)], 128, 128, kernel="ring"),
    "w256_one_tile": _w(1, [(3, 5)], 256, 256, kernel="w256"),
    "w256_k720": _w(2, [(13, 21)], 256, 720, kernel="w256"),
    "w256_k264_1x1": _w(2, [(9, 11)], 256, 264, R=1, kernel="w256"),
    "w256_k512_1x1_s2": _w(2, [(16, 24)], 256, 512, R=1, stride=2, kernel="w256"),
    "w9_one_tile": _w(1, [(3, 5)], 128, 128, kernel="w9"),
    "w9_k720": _w(2, [(13, 21)], 256, 720, kernel="w9"),
    "w9_k136": _w(1, [(9, 11)], 64, 136, kernel="w9"),
    "w9_widest_row": _w(2, [(7, 190)], 64, 128, kernel="w9"),
    "fold_k8": _w(2, [(10, 14), (5, 7), (3, 4), (2, 2)], 256, 8, kernel="fold"),
    "fold_k40": _w(2, [(10, 14), (5, 7), (3, 4), (2, 2)], 256, 40, kernel="fold"),
    "fold_k80": _w(2, [(10, 14), (5, 7), (3, 4), (2, 2)], 256, 80, kernel="fold"),
    "diag_s1": _w(2, [(9, 11)], 256, 256, kernel="diag", groups=32),
    "diag_s2": _w(2, [(14, 18)], 256, 256, stride=2, kernel="diag", groups=32),
}

ML_LEVELS = [(20, 28), (10, 14), (5, 7), (3, 4), (2, 2)]         # the multi-level cases: 64 -> 128, N = 2
SPLIT_LEVELS = [(16, 24), (5, 7)]                                # the split-dispatch cases: 256 -> 256, N = 2


def fwd_reference(c, form):
    """(ref, A, n, bf16) of one epilogue form of a forward case."""
    kw = dict(groups=c.groups, **c.geo)
    if form == "plain":
        return forward(c.x, c.w, **kw) + (True,)
    if form == "bias_relu":
        return forward(c.x, c.w, c.bias, relu=True, **kw) + (True,)
    if form in ("bias_res_relu", "bits"):
        return forward(c.x, c.w, c.bias, c.res, relu=True, **kw) + (True,)
    if form == "out_f32":
        return forward(c.x, c.w, c.bias, **kw) + (False,)
    if form in ("up2", "up2_f32"):
        return forward(c.x, c.w, c.bias, c.res_half, res_up2=True, **kw) + (form == "up2",)
    raise KeyError(form)


def dgrad_reference(c, form):
    kw = dict(groups=c.groups, **c.geo)
    hw = (c.H, c.W)
    if form == "plain":
        return dgrad(c.dy, c.w, hw, **kw)
    if form == "accum":
        return dgrad(c.dy, c.w, hw, accum=c.accum, **kw)
    if form == "mask":
        return dgrad(c.dy, c.w, hw, mask=c.mask, **kw)
    if form in ("accum_mask", "accum_bits"):
        return dgrad(c.dy, c.w, hw, accum=c.accum, mask=c.mask, **kw)
    if form == "accum_even":
        return dgrad(c.dy, c.w, hw, accum=c.accum_half, accum_even=True, mask=c.mask, **kw)
    raise KeyError(form)
