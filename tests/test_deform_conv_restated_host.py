"""CPU checks of tests/deform_conv_restated.py, for every case of its three tables:

* the restatement equals oracle/deform_conv.py and autograd through it, both in float64, to ``PIN * A`` per element (A = the
  element's absolute-addend sum; at integer positions autograd takes the floor-side derivative, the piece the kernels take);
* the two known-answer vectors of tests/golden/deform_conv_kat.npz;
* satisfiable: an fp32 emulation with bf16 roundings at the kernels' points (columns, column gradients, output) passes every check;
* sensitive: eight kinds of wrong answer are rejected wherever they apply.
"""
import copy
import os

import numpy as np
import pytest
import torch

import deform_conv_restated as D
from oracle import deform_conv as odc

PIN = 1e-12
G = os.path.join(os.path.dirname(__file__), "golden")
ALL = [(t, n) for t in ("FWD_CASES", "WGRAD_CASES", "BWD_CASES") for n in getattr(D, t)]
BWD = list(D.BWD_CASES)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _oracle_inputs(c, dtype):
    """The case in the oracle's layout.  In float64 the offsets are ``py - base`` of the restated (fp32-formed) positions, so the
    oracle samples exactly where the kernels do."""
    if dtype == torch.float64:
        by, bx = D.base_positions(c.Ho, c.Wo, c.ksize, c.stride, c.pad, c.dil)
        off = torch.stack([c.R.py - by, c.R.px - bx], dim=-1).reshape(c.N, c.Ho, c.Wo, -1)
    else:
        off = c.off
    x, off = _nchw(c.x.to(dtype)), _nchw(off.to(dtype))
    w = c.w.to(dtype).reshape(c.K, c.ksize[0], c.ksize[1], c.C).permute(0, 3, 1, 2).contiguous()
    mask = None if c.mask is None else _nchw(c.mask.to(dtype))
    return x, off, w, mask


def _oracle(c, dtype, hook=None, bias=False):
    """Oracle forward with leaves and the per-tap samples (NCHW, in the oracle's (g, i, j) order) recorded."""
    x, off, w, mask = (None if t is None else t.requires_grad_(True) for t in _oracle_inputs(c, dtype))
    samples = []

    def rec(s):
        samples.append(s)
        return hook(s) if hook is not None else s

    m = None if mask is None else (torch.sigmoid(mask) if c.logit else mask)
    y = odc.deform_conv2d(x, off, w, c.bias.to(dtype) if bias else None, c.stride, c.pad, c.dil, m, c.dg, sample_hook=rec)
    return y, x, off, w, mask, samples


def _samples_to_cols(samples, c):
    """[(N, cg, Ho, Wo)] in (g, tap) order -> (N, Ho, Wo, taps * C) with channel = tap * C + g * cg + c."""
    cg = c.C // c.dg
    t = torch.stack(samples, dim=0).reshape(c.dg, c.taps, c.N, cg, c.Ho, c.Wo)
    return t.permute(2, 4, 5, 1, 0, 3).reshape(c.N, c.Ho, c.Wo, c.taps * c.C)


def _w_like(c, gw):
    return gw.permute(0, 2, 3, 1).reshape(c.K, c.taps, c.C)


def _close(got, ref, A, what):
    err = (got.double() - ref).abs()
    assert bool((err <= PIN * A).all()), (what, float((err / A.clamp_min(1e-300)).max()))


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(table, name):
        if (table, name) not in cache:
            c = D.case(getattr(D, table), name)
            f = D.forward(c.x, c.R, c.w, c.mask, c.logit, c.bias)
            b = D.backward(c.x, c.R, c.w, c.dy, c.mask, c.logit)
            cache[(table, name)] = (c, f, b)
        return cache[(table, name)]
    return get


@pytest.mark.parametrize("table,name", ALL)
def test_floors_agree_and_restatement_is_the_oracle(cases, table, name):
    c, f, b = cases(table, name)
    assert c.R.floors_agree                       # fp32-formed and float64-formed positions fall in the same cell, on every sample
    y, x, off, w, mask, samples = _oracle(c, torch.float64, bias=True)
    leaves = [x, off, w] + ([mask] if mask is not None else [])
    g = torch.autograd.grad(y, leaves, _nchw(c.dy.double()))
    _close(_nhwc(y.detach()), f.y, f.A, "y")
    _close(_samples_to_cols([s.detach() for s in samples], c), f.cols, f.colsA, "cols")
    _close(_nhwc(g[0]), b.dx, b.dxA2, "dx")
    _close(_nhwc(g[1]), b.doff, b.doffA2, "d offset")
    _close(_w_like(c, g[2]), b.dw, b.dwA, "dW")
    if mask is not None:
        _close(_nhwc(g[3]), b.dmask, b.dmaskA2, "d mask")
    # the column gradient and the A1 / A2 order: |dcols| <= sum |dy| |w|
    assert bool((b.dcols.abs() <= b.dcolsA * (1 + 1e-12)).all()) and bool((b.dxA1 <= b.dxA2 * (1 + 1e-12) + 1e-300).all())


def test_known_answer_vectors():
    d = {k: torch.tensor(v) for k, v in np.load(os.path.join(G, "deform_conv_kat.npz")).items()}
    x = _nhwc(d["input"])
    w = d["weight"].permute(0, 2, 3, 1).reshape(1, 9, 2)
    for key, off in (("y_dconv_zero", "offsets_2"), ("y_dconv_1", "offsets_1")):
        R = D.restate(_nhwc(d[off]), 4, 4, (3, 3), 1, 1, 1, 1)
        f = D.forward(x, R, w)
        np.testing.assert_allclose(f.y[0, :, :, 0].numpy(), d[key][0, 0].numpy(), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------ satisfiable
def _emulate(c):
    """What a correct kernel family computes, in fp32 with the bf16 roundings at the kernels' points (none in the fp32 mode)."""
    f32 = c.f32
    r = (lambda t: t) if f32 else D.rb
    y, x, off, w, mask, samples = _oracle(c, torch.float32, hook=r, bias=True)
    leaves = [x, off] + ([mask] if mask is not None else [])
    (dw,) = torch.autograd.grad(y, [w], _nchw(c.dy), retain_graph=True)
    cols = _samples_to_cols([s.detach() for s in samples], c)
    dcols = r(torch.einsum("nhwk,ktc->nhwtc", c.dy, c.w).reshape(c.N, c.Ho, c.Wo, -1))          # fp32 contraction, stored as bf16
    cg = c.C // c.dg
    gs = [_nchw(dcols.reshape(c.N, c.Ho, c.Wo, c.taps, c.dg, cg)[:, :, :, t, g]) for g in range(c.dg) for t in range(c.taps)]
    g = torch.autograd.grad(samples, leaves, gs)
    return dict(y=_nhwc(y.detach()), cols=r(cols), dw=_w_like(c, dw), dx=_nhwc(g[0]), doff=_nhwc(g[1]), dmask=_nhwc(g[2]) if mask is not None else None,
                f32=f32, dcols=dcols)


def _qsum(c, b, path):
    if path == "tiled":
        return D.dx_quantum_sum(D.quantum_tiled(b.dcols, c.R, c.mask, c.logit), c.R)
    if path == "fused":
        return D.dx_quantum_sum(D.quantum_fused(c.dy, c.w, c.R, c.mask, c.logit), c.R)
    return None


@pytest.mark.parametrize("table,name", ALL)
def test_an_fp32_emulation_with_bf16_roundings_passes(cases, table, name):
    c, f, b = cases(table, name)
    e = _emulate(c)
    mode = "f32" if e["f32"] else "bf16"
    out = {}
    if e["f32"]:
        out["y"] = D.check_fwd(e["y"], f, "f32")
    else:
        out["y f32"] = D.check_fwd(e["y"], f, "out_f32")
        out["y"] = D.check_fwd(D.rb(e["y"]), f, "bf16")
        fr = copy.copy(f)
        fr.y = torch.relu(f.y)
        out["y relu"] = D.check_fwd(D.rb(torch.relu(e["y"])), fr, "bf16")
    out["cols"] = D.check_cols(e["cols"], f, mode)
    if not e["f32"]:
        out["dw"] = D.check_dw(e["dw"], b)
    out["dx"] = D.check_dx(e["dx"], b, None, mode)            # no quantum term: the emulation has no fixed point
    out["doff"] = D.check_doff(e["doff"], b, mode)
    if c.mask is not None:
        out["dmask"] = D.check_dmask(e["dmask"], b, mode)
    print(name, {k: "%.3f" % v["ratio"] for k, v in out.items()})
    assert all(v["compared"] > 0 for v in out.values())


# ------------------------------------------------------------------ sensitive
def _mutated_R(c, kind):
    R = copy.copy(c.R)
    H, W = R.H, R.W
    if kind == "closed_valid":                    # 1: >= / <= in place of > / <
        valid = (R.py >= -1) & (R.px >= -1) & (R.py <= H) & (R.px <= W)
        fy, fx = R.py.floor(), R.px.floor()
        ok = []
        for dyc in (0, 1):
            for dxc in (0, 1):
                yy, xx = fy + dyc, fx + dxc
                ok.append(valid & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1))
        R.valid, R.ok = valid, torch.stack(ok)
    elif kind == "no_high_corner":                # 2: the yh / xh corner dropped for samples in (-1, 0)
        by_, bx_ = (R.py > -1) & (R.py < 0), (R.px > -1) & (R.px < 0)
        ok = R.ok.clone()
        ok[2] &= ~by_
        ok[3] &= ~(by_ | bx_)
        ok[1] &= ~bx_
        R.ok = ok
    return R


def _applies(c, kind):
    R = c.R
    inx, iny = (R.px > -1) & (R.px < R.W), (R.py > -1) & (R.py < R.H)
    if kind == "closed_valid":
        return bool((((R.py == -1) & inx & (R.px >= 0)) | ((R.px == -1) & iny & (R.py >= 0))).any())
    if kind == "no_high_corner":
        return bool((R.valid & ((R.py < 0) | (R.px < 0))).any())
    if kind == "swap_last_group":
        return True
    if kind == "mask_of_group0":
        return c.mask is not None and c.dg > 1
    if kind == "transposed_taps":
        return c.taps > 1
    if kind == "skipped_edge":
        return c.Ho % D.TILE != 0 or c.Wo % D.TILE != 0
    raise ValueError(kind)


def _wrong(c, kind):
    """The float64 results of one wrong rule (forward and all gradients)."""
    off, mask, R, keep = c.off, c.mask, c.R, None
    o = c.off.reshape(c.N, c.Ho, c.Wo, c.dg, c.taps, 2).clone()
    if kind in ("closed_valid", "no_high_corner"):
        R = _mutated_R(c, kind)
    elif kind == "swap_last_group":               # 3
        o[:, :, :, c.dg - 1] = o[:, :, :, c.dg - 1].flip(-1)
        R = D.restate(o.reshape(c.off.shape), c.H, c.W, c.ksize, c.stride, c.pad, c.dil, c.dg)
    elif kind == "mask_of_group0":                # 4
        m = c.mask.reshape(c.N, c.Ho, c.Wo, c.dg, c.taps)
        mask = m[:, :, :, :1].expand(-1, -1, -1, c.dg, -1).reshape(c.mask.shape)
    elif kind == "transposed_taps":               # 5: base (kj, ki) in place of (ki, kj)
        t = torch.arange(c.taps)
        ki, kj = t // c.ksize[1], t % c.ksize[1]
        o[..., 0] += ((kj - ki) * c.dil).float()
        o[..., 1] += ((ki - kj) * c.dil).float()
        R = D.restate(o.reshape(c.off.shape), c.H, c.W, c.ksize, c.stride, c.pad, c.dil, c.dg)
    elif kind == "skipped_edge":                  # 6: the last row and column of a partial 8x8 tile
        keep = torch.ones(c.N, c.Ho, c.Wo, dtype=torch.bool)
        if c.Ho % D.TILE:
            keep[:, c.Ho - 1] = False
        if c.Wo % D.TILE:
            keep[:, :, c.Wo - 1] = False
    f = D.forward(c.x, R, c.w, mask, c.logit, c.bias)
    if keep is not None:
        f.y = f.y * keep.unsqueeze(-1)
    b = D.backward(c.x, R, c.w, c.dy, mask, c.logit, keep_pixels=keep)
    return f, b


KINDS = ("closed_valid", "no_high_corner", "swap_last_group", "mask_of_group0", "transposed_taps", "skipped_edge")


@pytest.mark.parametrize("table,name", ALL)
def test_wrong_rules_are_rejected(cases, table, name):
    c, f, b = cases(table, name)
    path = getattr(c, "path", None)
    qs = _qsum(c, b, path)
    mode = "f32" if c.f32 else "bf16"
    applied = []
    for kind in KINDS:
        if not _applies(c, kind):
            continue
        applied.append(kind)
        wf, wb = _wrong(c, kind)
        if kind == "closed_valid":                # a sample at exactly -1 has weight zero on its only live corners: the value does not
            r = D.check_doff(wb.doff, b, mode, enforce=False)     # change, its derivative does
            assert r["ratio"] > 1, (kind, r)
            continue
        if table == "FWD_CASES":
            r = D.check_fwd(wf.y, f, mode, enforce=False)
        elif table == "WGRAD_CASES":
            r = D.check_dw(wb.dw, b, enforce=False)
        else:
            r = D.check_dx(wb.dx, b, qs, mode, enforce=False)
        assert r["ratio"] > 1, (kind, r)
    print(name, applied)
    assert "swap_last_group" in applied


def test_every_wrong_rule_applies_somewhere():
    for kind in KINDS:
        for table in ("FWD_CASES", "BWD_CASES"):
            assert any(_applies(D.case(getattr(D, table), n), kind) for n in getattr(D, table)), (kind, table)


@pytest.mark.parametrize("name", [n for n in BWD if D.BWD_CASES[n]["path"] in ("tiled", "fused")])
def test_a_wrapped_window_cell_is_rejected(cases, name):
    """7: one cell's int32 sum wrapped modulo 2^32 - the cell is off by 2^32 quanta of its tile (half of that with the ex + 1 allowance)."""
    c, f, b = cases("BWD_CASES", name)
    path = c.path
    qpix = D.quantum_tiled(b.dcols, c.R, c.mask, c.logit) if path == "tiled" else D.quantum_fused(c.dy, c.w, c.R, c.mask, c.logit)
    qs = D.dx_quantum_sum(qpix, c.R)
    assert bool((qs > 0).any())
    assert D.check_dx(b.dx, b, qs, enforce=False)["ratio"] == 0
    cell = torch.nonzero(b.dx.abs() == b.dx.abs().max())[0]
    wrong = b.dx.clone()
    wrong[tuple(cell)] -= torch.sign(wrong[tuple(cell)]) * 2.0 ** 32 * float(qpix[qpix > 0].min()) / 2
    assert D.check_dx(wrong, b, qs, enforce=False)["ratio"] > 1


@pytest.mark.parametrize("name", [n for n in BWD if D.BWD_CASES[n].get("mask") == "zero_tile"])
def test_a_mask_gradient_dropped_on_a_zero_mask_tile_is_rejected(cases, name):
    """8: d mask = sum_c dcols * sample does not vanish where the mask does."""
    c, f, b = cases("BWD_CASES", name)
    m = c.mask.reshape(c.N, c.Ho, c.Wo, c.dg, c.taps)
    assert bool((m[:, :D.TILE, :D.TILE, c.dg - 1] == 0).all())
    wrong = b.dmask.reshape(m.shape).clone()
    assert float(wrong[:, :D.TILE, :D.TILE, c.dg - 1].abs().max()) > 0
    wrong[:, :D.TILE, :D.TILE, c.dg - 1] = 0
    assert D.check_dmask(wrong.reshape(b.dmask.shape), b, enforce=False)["ratio"] > 1
    assert D.check_dmask(b.dmask, b)["ratio"] == 0


def test_quantum_rule():
    assert (D.fbits(9), D.fbits(1), D.fbits(25)) == (20, 24, 19)
    q = D._quantum_of(torch.tensor([0.0, 0.75, 1.0, float("inf"), float("nan")], dtype=torch.float64), 9)
    assert q.tolist() == [0.0, 2.0 ** (0 + 1 - 20), 2.0 ** (1 + 1 - 20), 0.0, 0.0]


def test_non_finite_sets_must_match():
    ref = torch.tensor([1.0, float("nan"), 2.0], dtype=torch.float64)
    bound = torch.ones(3, dtype=torch.float64)
    assert D._measure(torch.tensor([1.0, float("nan"), 2.0]), ref, bound, "x", False)["same_nonfinite"]
    assert not D._measure(torch.tensor([1.0, 0.0, 2.0]), ref, bound, "x", False)["same_nonfinite"]
    assert not D._measure(torch.tensor([float("nan"), float("nan"), 2.0]), ref, bound, "x", False)["same_nonfinite"]
    with pytest.raises(AssertionError):
        D._measure(torch.tensor([1.0, 0.0, 2.0]), ref, bound, "x", True)
