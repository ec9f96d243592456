"""GPU parity of FCOSRepPoints (slender_det/modeling/meta_arch/fcos/fcos_rpd_s1_topk.py): the slender top-k assignment, the points -> LTRB
transform, the batched refine targets, the linear-LTRB decode and the loss finalisation against the fixtures the reference's own Python
produced (tests/golden/fcos_reppoints/) and against the restatement (tests/fcos_reppoints_restated.py, pinned to those fixtures by
tests/test_fcos_reppoints_host.py); the model against the oracle.

Bars (the project's existing ones): labels, regression targets, gt indices, selections, matches and matcher labels are exact; scores 1e-6
of max|ref|, stats 1e-5 with the counts exact; the transform's forward exact, its fp32 backward 1e-6, bf16 rows 2^-7, d(scale) 1e-4;
the four losses 2e-5, loss gradients 2^-7 of max|ref| per tensor; decoded scores 1e-6 and boxes 1e-5 of max|box|; the fp32-mode step
2e-5 per loss and the 1e-4 / 90 %-within-2e-5 gradient rule of test_gpu_f32_mode; the bf16 step 1e-3 (the README's parity bar)."""
import os

import numpy as np
import pytest
import torch

import fcos_reppoints_restated as RS
from oracle import fcos_targets as ot
from oracle import losses as ol
from test_fcos_reppoints_host import SLENDER_BOX
from test_gpu_fcos_topk import _assert_gradients_tight, _cpu, _forced_oracle_grads, _tapped_step

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_reppoints")
HW = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]          # 128 x 160 padded, L = 428
STRIDES = [8, 16, 32, 64, 128]
L = sum(h * w for h, w in HW)
THR, LAB = [0.4, 0.5], [0, -1, 1]


def _rel(got, ref, tol, what):
    got = got.detach().float().cpu().reshape(-1)
    ref = ref.detach().float().reshape(-1)
    err = (got - ref).abs().max().item()
    lim = tol * max(ref.abs().max().item(), 1e-6)
    print(f"{what}: err {err:.4g} (limit {lim:.4g})")
    assert err <= lim, f"{what}: err {err:.4g} > {lim:.4g}"


def _load_gts(z):
    n = len([k for k in z.files if k.startswith("boxes")])
    return [torch.from_numpy(z[f"boxes{i}"]) for i in range(n)], [torch.from_numpy(z[f"classes{i}"]) for i in range(n)]


def _gt_tensors(cuda, boxes, classes):
    offs = torch.tensor([0] + [len(b) for b in boxes]).cumsum(0).int()
    if sum(len(b) for b in boxes):
        allb, allc = torch.cat([b.reshape(-1, 4) for b in boxes]).float(), torch.cat(classes).int()
    else:
        allb, allc = torch.zeros(1, 4), torch.zeros(1).int()
    return allb.to(cuda), allc.to(cuda), offs.to(cuda)


def _assign(cuda, boxes, classes, radius, K=80, topk=5, slender=True):
    from slenderobjdet_amd.layers import functional as HF

    allb, allc, offs = _gt_tensors(cuda, boxes, classes)
    return HF.fcos_assign_topk(allb, allc, offs, len(boxes), HW, STRIDES, ot.SIZES_OF_INTEREST, radius, K, topk, slender=slender)


def _check_against_restatement(cuda, boxes, classes, radius, K=80, topk=5):
    """Kernel == restatement, exactly, on everything discrete; returns the restatement's and the kernel's outputs."""
    ref = RS.slender_targets(HW, STRIDES, boxes, classes, radius, K, topk)
    lab, reg, ctr, idx, sel, stats = (t.cpu() for t in _assign(cuda, boxes, classes, radius, K, topk))
    assert torch.equal(lab.long(), ref[0]), "labels"
    assert torch.equal(reg, ref[1]), "regression targets"
    assert torch.equal(idx.long(), ref[3]), "gt_index"
    assert sel.dtype == torch.uint8 and torch.equal(sel.bool(), ref[4]), "selection"
    _rel(ctr, ref[2], 1e-6, "slender scores")
    fg = ref[0] != K
    assert float(stats[0]) == float(fg.sum())
    _rel(stats, torch.stack([fg.sum().float(), ref[2][ref[4]].sum(), ref[2].sum()]), 1e-5, "stats3")
    return ref, (lab, reg, ctr, idx, sel, stats)


# ------------------------------------------------------------------------------------------------ 1. assignment
@pytest.mark.parametrize("name", ["targets_seed1.npz", "targets_seed2.npz"])
@pytest.mark.parametrize("radius", [1.5, 0.0])
def test_slender_assignment_equals_the_reference(cuda, name, radius):
    z = np.load(os.path.join(GOLD, name))
    boxes, classes = _load_gts(z)
    assert [tuple(int(v) for v in r) for r in z["level_hw"]] == HW
    ref, (lab, reg, ctr, idx, sel, stats) = _check_against_restatement(cuda, boxes, classes, radius)
    assert torch.equal(lab.long(), torch.from_numpy(z[f"gt_classes_r{radius}"]))
    assert torch.equal(reg, torch.from_numpy(z[f"reg_targets_r{radius}"]))
    assert torch.equal(sel.bool(), torch.from_numpy(z[f"topk_locations_r{radius}"]))
    _rel(ctr, torch.from_numpy(z[f"scores_r{radius}"]), 1e-6, "slender scores vs the reference")
    fg = lab != 80
    assert bool((idx[~fg] == -1).all()) and 0 < int(sel.sum()) < int(fg.sum())
    # labels, regression targets and gt indices are those of sod_fcos_assign_topk, bit for bit; the scores are not
    plain = [t.cpu() for t in _assign(cuda, boxes, classes, radius, slender=False)]
    assert torch.equal(plain[0], lab) and torch.equal(plain[1], reg) and torch.equal(plain[3], idx)
    assert float(plain[5][0]) == float(stats[0]) and not torch.equal(plain[2], ctr)


def test_selection_differs_from_the_plain_top_k_on_a_slender_box(cuda):
    """See tests/test_fcos_reppoints_host.py::test_slender_selection_differs_from_the_plain_one_on_a_slender_box: w / h is constant inside
    a box, so the two scores order the positives alike and the selections part only where rounding decides; on this box the restatement's
    do (353 against 355), and each kernel follows its restatement."""
    boxes, classes = [torch.tensor([SLENDER_BOX])], [torch.tensor([3])]
    a = RS.slender_targets(HW, STRIDES, boxes, classes, 0.0, 80)
    b = RS.slender_targets(HW, STRIDES, boxes, classes, 0.0, 80, score=ol.centerness_targets)
    assert not torch.equal(a[4], b[4])
    ka = [t.cpu() for t in _assign(cuda, boxes, classes, 0.0)]
    kb = [t.cpu() for t in _assign(cuda, boxes, classes, 0.0, slender=False)]
    print("slender scores of 353 / 355:", float(ka[2][0, 353]).hex(), float(ka[2][0, 355]).hex(), "restated", float(a[2][0, 353]).hex())
    assert torch.equal(kb[4].bool(), b[4]), "plain selection"
    assert torch.equal(ka[4].bool(), a[4]), "slender selection"
    assert not torch.equal(ka[4], kb[4])
    _rel(ka[2], a[2], 1e-6, "slender scores")


def _t(*rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4)


def _c(*v):
    return torch.tensor(v, dtype=torch.int64)


def test_box_with_no_more_than_k_positives_selects_all(cuda):
    ref, (lab, _r, _c_, _i, sel, _s) = _check_against_restatement(cuda, [_t([10, 10, 24, 22])], [_c(4)], 0.0)
    assert int((lab != 80).sum()) == 4 and int(sel.sum()) == 4


def test_empty_image_between_two_others_and_an_all_empty_batch(cuda):
    boxes = [_t([8.5, 8.5, 72.25, 72.5]), _t(), _t([30.25, 20.5, 140.0, 100.5], [5.0, 60.25, 40.5, 120.0])]
    ref, (lab, _r, _c_, idx, sel, _s) = _check_against_restatement(cuda, boxes, [_c(1), _c(), _c(2, 3)], 1.5)
    assert bool((lab[1] == 80).all()) and bool((idx[1] == -1).all()) and int(sel[1].sum()) == 0
    assert set(idx[2][idx[2] >= 0].tolist()) == {1, 2}                       # indices into the CONCATENATED gt list
    ref, (lab, reg, ctr, idx, sel, stats) = _check_against_restatement(cuda, [_t(), _t()], [_c(), _c()], 1.5)
    assert bool((lab == 80).all()) and bool((idx == -1).all()) and int(sel.sum()) == 0 and bool((stats == 0).all())


def test_more_boxes_than_lanes_in_a_wave(cuda):
    boxes = _t(*[[16 * j + 1.25, 18 * i + 1.5, 16 * j + 15.0, 18 * i + 17.25] for i in range(7) for j in range(10)])
    ref, (lab, _r, _c_, idx, sel, _s) = _check_against_restatement(cuda, [_t([3.5, 2.25, 60.0, 50.5]), boxes], [_c(7), torch.arange(70) % 80], 0.0)
    owners = set(idx[1][idx[1] >= 0].tolist())
    assert len(owners) == 70 and max(owners) == 70


def test_tie_at_the_cut_takes_the_lower_location(cuda):
    """Box (8, 8, 40, 40), radius 0: a square, so the exponent is 1 and the score is the plain product: 4 x 0.36, 8 x 0.0857, 4 x 0.0204 on
    the stride-8 level.  The four 0.36 and the lowest-index 0.0857."""
    ref, (lab, _r, ctr, _i, sel, _s) = _check_against_restatement(cuda, [_t([8, 8, 40, 40])], [_c(3)], 0.0)
    pos = (lab[0] != 80).nonzero().squeeze(1)
    vals = ctr[0, pos]
    assert pos.numel() == 16 and int((vals > 0.3).sum()) == 4
    mid = pos[(vals > 0.05) & (vals < 0.3)]
    assert mid.numel() == 8 and len(set(vals[(vals > 0.05) & (vals < 0.3)].tolist())) == 1          # an exact eight-way tie on the device
    assert set(sel[0].nonzero().squeeze(1).tolist()) == set(pos[vals > 0.3].tolist()) | {int(mid.min())}


@pytest.mark.parametrize("topk", [1, 8])
def test_other_k(cuda, topk):
    z = np.load(os.path.join(GOLD, "targets_seed1.npz"))
    boxes, classes = _load_gts(z)
    ref, (lab, _r, _c_, idx, sel, _s) = _check_against_restatement(cuda, boxes, classes, 0.0, topk=topk)
    per_gt = [int(sel[idx == g].sum()) for g in range(sum(len(b) for b in boxes))]
    assert max(per_gt) == topk


def test_stats_are_reproducible_and_topk_range_is_checked(cuda):
    from slenderobjdet_amd import _C

    z = np.load(os.path.join(GOLD, "targets_seed2.npz"))
    boxes, classes = _load_gts(z)
    a = _assign(cuda, boxes, classes, 1.5)
    b = _assign(cuda, boxes, classes, 1.5)
    assert torch.equal(a[5], b[5]) and torch.equal(a[4], b[4])
    for k in (0, 9):
        with pytest.raises(_C.SlenderHipError):
            _assign(cuda, boxes, classes, 1.5, topk=k)


# ------------------------------------------------------------------------------------------------ 2. points -> LTRB
def _rows(per_level, ld=24):
    """Per-level (N, 18, H, W) point offsets -> the product's fp32 rows (N, H, W, ld), zero padded."""
    out = []
    for t in per_level:
        r = torch.zeros(t.shape[0], t.shape[2], t.shape[3], ld)
        r[..., : t.shape[1]] = t.permute(0, 2, 3, 1)
        out.append(r.contiguous())
    return out


def _p2l(cuda, pts_rows, add_rows=None, boxes=True):
    from slenderobjdet_amd.layers import functional as HF

    N = pts_rows[0].shape[0]
    ltrb = torch.full((N, L, 4), 7.0, device=cuda)
    bx = torch.full((N, L, 4), 7.0, device=cuda) if boxes else None
    arg = torch.zeros((N, L), dtype=torch.int32, device=cuda)
    o = 0
    for l, (h, w) in enumerate(HW):
        add = add_rows[l].to(cuda) if add_rows is not None else None
        HF.points2ltrb_fwd(pts_rows[l].to(cuda), add, STRIDES[l], RS.POINT_STRIDES[l], 9, ltrb.view(-1)[o * 4:], bx.view(-1)[o * 4:] if boxes else None,
                           L * 4, arg.view(-1)[o:], L)
        o += h * w
    return ltrb, bx, arg


def _p2l_bwd(cuda, d, arg, N, bf16=False):
    from slenderobjdet_amd.layers import functional as HF

    out, o = [], 0
    for l, (h, w) in enumerate(HW):
        d32, d16 = HF.points2ltrb_bwd(d.view(-1)[o * 4:], L * 4, arg.view(-1)[o:], L, (N, h, w, 24), RS.POINT_STRIDES[l], 9, want_f32=True, want_bf16=bf16)
        out.append((d32, d16))
        o += h * w
    return out


def test_points2ltrb_forward_equals_the_reference(cuda):
    z = np.load(os.path.join(GOLD, "offsets2ltrb.npz"))
    pts = [torch.from_numpy(z[f"points{l}"]) for l in range(len(HW))]
    ref = RS.ltrb_rows([torch.from_numpy(z[f"ltrb{l}"]) for l in range(len(HW))])
    assert torch.equal(RS.ltrb_rows(RS.offsets2ltrb(pts)), ref)
    ltrb, boxes, _arg = _p2l(cuda, _rows(pts))
    assert torch.equal(ltrb.cpu(), ref), "LTRB"
    assert torch.equal(boxes.cpu(), RS.decode_boxes(ref, HW, STRIDES)), "decoded boxes"
    # offsets_refine + offsets_init.detach(): the second addend
    add = [torch.randn(p.shape, generator=torch.Generator().manual_seed(5)) for p in pts]
    ltrb2, _b, _a = _p2l(cuda, _rows(pts), _rows(add), boxes=False)
    assert torch.equal(ltrb2.cpu(), RS.ltrb_rows(RS.offsets2ltrb([p + a for p, a in zip(pts, add)])))


def test_points2ltrb_backward_and_scale(cuda):
    from slenderobjdet_amd.layers import functional as HF

    g = torch.Generator().manual_seed(7)
    raw = [torch.randn(2, 18, h, w, generator=g) * 3 for h, w in HW]
    scales = torch.tensor([1.0, 0.9, 1.1, 1.2, 0.8])
    w4 = torch.randn(2, L, 4, generator=g)
    rawr, sc = [r.clone().requires_grad_(True) for r in raw], scales.clone().requires_grad_(True)
    ref_ltrb = RS.ltrb_rows(RS.offsets2ltrb([r * sc[l] for l, r in enumerate(rawr)]))
    grads = torch.autograd.grad((ref_ltrb * w4).sum(), rawr + [sc])
    rows = _rows(raw)
    scaled = [HF.level_scale_fwd(rows[l].to(cuda), scales[l:l + 1].to(cuda)) for l in range(len(HW))]
    for l in range(len(HW)):
        assert torch.equal(scaled[l].cpu(), rows[l] * scales[l])
    ltrb, _b, arg = _p2l(cuda, [s.cpu() for s in scaled], boxes=False)
    assert torch.equal(ltrb.cpu(), ref_ltrb.detach())
    back = _p2l_bwd(cuda, w4.to(cuda), arg, 2, bf16=True)
    dsc = torch.zeros(5, device=cuda)
    for l in range(len(HW)):
        d32, d16 = back[l]
        dpts = (grads[l] / scales[l]).permute(0, 2, 3, 1)            # d(scaled points) = d(raw) / scale
        _rel(d32[..., :18], dpts, 1e-6, f"d(points) level {l}")
        _rel(d16[..., :18], dpts, 2 ** -7, f"d(points) bf16 level {l}")
        assert (d32[..., 18:] == 0).all() and (d16[..., 18:] == 0).all()
        draw = HF.level_scale_bwd(d32, rows[l].to(cuda), scales[l:l + 1].to(cuda), dsc[l:l + 1])
        _rel(draw[..., :18], grads[l].permute(0, 2, 3, 1), 1e-6, f"d(raw points) level {l}")
    _rel(dsc, grads[-1], 1e-4, "d(scale)")
    dsc2 = dsc.clone()
    for l in range(len(HW)):            # accumulates, in a fixed order
        HF.level_scale_bwd(back[l][0], rows[l].to(cuda), scales[l:l + 1].to(cuda), dsc2[l:l + 1])
    assert torch.equal(dsc2, dsc * 2)


def test_points2ltrb_two_points_share_the_minimum(cuda):
    """Points 2 and 6 share the smallest x, points 1 and 4 the largest y: the LOWEST index wins, which is the index ``torch.min`` /
    ``torch.max`` over the point dimension return on the CPU and therefore where the restatement's gradient goes."""
    pts = [torch.zeros(1, 18, h, w) for h, w in HW]
    for p in pts:
        p[:, 0::2] = torch.tensor([0.5, 1.0, -2.0, 0.0, 1.5, 0.25, -2.0, 1.0, 0.75]).view(1, 9, 1, 1)
        p[:, 1::2] = torch.tensor([0.5, 3.0, -1.0, 0.0, 3.0, 0.25, -0.5, 1.0, 0.75]).view(1, 9, 1, 1)
    pr = [p.clone().requires_grad_(True) for p in pts]
    ref = RS.ltrb_rows(RS.offsets2ltrb(pr))
    grads = torch.autograd.grad(ref.sum(), pr)
    assert float(grads[0][0, 4, 0, 0]) == -1.0 and float(grads[0][0, 12, 0, 0]) == 0.0           # x of point 2, not of point 6
    assert float(grads[0][0, 3, 0, 0]) == 1.0 and float(grads[0][0, 9, 0, 0]) == 0.0            # y of point 1, not of point 4
    ltrb, _b, arg = _p2l(cuda, _rows(pts), boxes=False)
    assert torch.equal(ltrb.cpu(), ref.detach())
    assert int(arg[0, 0]) == (2 | (2 << 8) | (4 << 16) | (1 << 24))
    back = _p2l_bwd(cuda, torch.ones(1, L, 4, device=cuda), arg, 1)
    for l in range(len(HW)):
        assert torch.equal(back[l][0][..., :18].cpu(), grads[l].permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------ 3. refine targets
def _refine(cuda, boxes, classes, cand, sizes, K=80):
    from slenderobjdet_amd.layers import functional as HF

    allb, allc, offs = _gt_tensors(cuda, boxes, classes)
    hw = torch.tensor([[float(h), float(w)] for h, w in sizes]).to(cuda)
    return HF.fcos_rpd_refine_targets(allb, allc, offs, [len(b) for b in boxes], cand.to(cuda).contiguous(), hw, HW, STRIDES, K, THR, LAB, True)


def _check_refine(cuda, boxes, classes, cand, sizes, K=80):
    """The batched entry point == N calls of sod_anchor_match + the label rule, bit for bit, and == the restatement."""
    from slenderobjdet_amd.layers import functional as HF

    vals, matches, mlab, cls, cls_bg, ltrb = _refine(cuda, boxes, classes, cand, sizes, K)
    loc = torch.cat(ot.locations(HW, STRIDES))
    for i, (b, c) in enumerate(zip(boxes, classes)):
        v1, m1, l1 = HF.anchor_match(b.reshape(-1, 4).float().to(cuda), cand[i].to(cuda).contiguous(), THR, LAB, True)
        assert torch.equal(v1, vals[i]) and torch.equal(m1, matches[i]) and torch.equal(l1, mlab[i]), i
        h, w = sizes[i]
        want = c[m1.cpu().long()].clone().long() if len(b) else torch.full((L,), K)
        want[l1.cpu() == 0] = K
        want[(loc[:, 0] >= w) | (loc[:, 1] >= h)] = -1
        assert torch.equal(cls[i].cpu().long(), want), i
    ref = RS.refine_targets(HW, STRIDES, cand, boxes, classes, sizes, K, THR, LAB)
    assert torch.equal(cls.cpu().long(), ref[0]) and torch.equal(ltrb.cpu(), ref[1])
    assert torch.equal(matches.cpu().long(), ref[2]) and torch.equal(mlab.cpu(), ref[3])
    _rel(vals, ref[4], 1e-6, "matched IoU")
    assert torch.equal(cls_bg.cpu(), torch.where(cls.cpu() < 0, torch.full_like(cls.cpu(), K), cls.cpu()))
    return cls.cpu(), ltrb.cpu(), mlab.cpu(), vals.cpu()


def test_refine_targets_equal_the_reference(cuda):
    z = np.load(os.path.join(GOLD, "ground_truth.npz"))
    boxes, classes = _load_gts(z)
    sizes = [tuple(int(v) for v in r) for r in z["image_sizes"]]
    cls, ltrb, mlab, _v = _check_refine(cuda, boxes, classes, torch.from_numpy(z["init_boxes"]), sizes)
    assert torch.equal(cls.long(), torch.from_numpy(z["refine_gt_classes"])) and torch.equal(ltrb, torch.from_numpy(z["refine_reg_targets"]))
    assert int((cls[1] == -1).sum()) > 40 and int(((cls >= 0) & (cls != 80)).sum()) > sum(len(b) for b in boxes)


def test_refine_targets_70_boxes_in_one_image_none_in_another(cuda):
    many = _t(*[[16 * j + 1.25, 18 * i + 1.5, 16 * j + 15.0, 18 * i + 17.25] for i in range(7) for j in range(10)])
    boxes, classes = [many, _t(), _t([30.25, 20.5, 140.0, 100.5])], [torch.arange(70) % 80, _c(), _c(5)]
    g = torch.Generator().manual_seed(11)
    loc = torch.cat(ot.locations(HW, STRIDES))
    st = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(HW, STRIDES)])
    d = (torch.rand(3, L, 4, generator=g) * 1.5 + 0.3) * st[None, :, None]
    cand = torch.stack([loc[None, :, 0] - d[..., 0], loc[None, :, 1] - d[..., 1], loc[None, :, 0] + d[..., 2], loc[None, :, 1] + d[..., 3]], dim=2)
    cls, ltrb, mlab, _v = _check_refine(cuda, boxes, classes, cand, [(128, 160), (128, 150), (128, 160)])
    assert len(set(cls[0][(cls[0] >= 0) & (cls[0] != 80)].tolist())) > 30
    outside = loc[:, 0] >= 150
    assert bool((cls[1][~outside] == 80).all()) and bool((cls[1][outside] == -1).all()) and bool((ltrb[1] == 0).all()) and bool((mlab[1] == 0).all())


def test_low_quality_rule_keeps_a_gt_whose_best_iou_is_small(cuda):
    """One 40 x 40 gt, candidates of 12.7 x 12.7 around every location: the best IoU is ~0.1, below both thresholds, and the candidate
    that attains it is still positive (allow_low_quality_matches)."""
    loc = torch.cat(ot.locations(HW, STRIDES))
    cand = torch.cat([loc - 6.35, loc + 6.35], dim=1)[None].contiguous()
    boxes, classes = [_t([30.5, 41.0, 70.5, 81.0])], [_c(9)]
    cls, _ltrb, mlab, vals = _check_refine(cuda, boxes, classes, cand, [(128, 160)])
    pos = ((cls >= 0) & (cls != 80)).nonzero()
    assert 0.05 < float(vals.max()) < 0.15 and pos.shape[0] >= 1 and bool((cls[(cls != 80) & (cls >= 0)] == 9).all())
    assert bool((vals[0, pos[:, 1]] == vals.max()).all()) and bool((mlab[0, pos[:, 1]] == 1).all())


# ------------------------------------------------------------------------------------------------ 4. decode
def test_decode_ltrb_equals_the_exp_decode_and_the_restatement(cuda):
    from slenderobjdet_amd.layers import functional as HF

    g = torch.Generator().manual_seed(3)
    N, K, top_n = 2, 8, 30
    logits = (torch.randn(N, L, K, generator=g) * 2 - 1).contiguous()
    ctr = torch.randn(N, L, 8, generator=g).contiguous()
    st = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(HW, STRIDES)])
    d = ((torch.rand(N, L, 4, generator=g) * 3 + 0.2) * st[None, :, None]).contiguous()
    raw = torch.zeros(N, L, 8)
    raw[..., :4], raw[..., 4] = torch.log(d), ctr[..., 0]
    a = HF.fcos_decode(logits.to(cuda), raw.to(cuda), torch.ones(5, device=cuda), HW, STRIDES, K, True, False, 0.3, top_n)
    b = HF.fcos_decode_ltrb(logits.to(cuda), d.to(cuda), ctr.to(cuda), HW, STRIDES, K, 0.3, top_n)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and int(b[3].max()) == top_n and int(b[3].min()) < top_n
    valid = torch.isfinite(a[1])
    assert torch.equal(valid, torch.isfinite(b[1]))
    _rel(b[1][valid], a[1][valid].cpu(), 1e-6, "scores")
    _rel(b[0], a[0].cpu(), 1e-5, "boxes")
    # negative distances: against the restatement
    d2 = d.clone()
    d2[:, ::3, 0] *= -0.5
    d2[:, 1::4, 3] *= -0.25
    boxes, scores, classes, counts = (t.cpu() for t in HF.fcos_decode_ltrb(logits.to(cuda), d2.to(cuda), ctr.to(cuda), HW, STRIDES, K, 0.3, top_n))
    for n in range(N):
        ref = RS.decode_ltrb(logits[n], d2[n], ctr[n, :, 0], HW, STRIDES, 0.3, top_n)
        for l, (rb, rs, rc) in enumerate(ref):
            c = int(counts[n, l])
            sl = slice(l * top_n, l * top_n + c)
            assert c == len(rs) and torch.equal(classes[n, sl].long(), rc), (n, l)
            assert torch.equal(boxes[n, sl], rb), (n, l)
            _rel(scores[n, sl], rs, 1e-6, f"scores image {n} level {l}")
            assert bool(torch.isinf(scores[n, l * top_n + c:(l + 1) * top_n]).all())
    assert bool((boxes[..., 2] < boxes[..., 0]).any())          # a box turned inside out by a negative distance comes out as it is


# ------------------------------------------------------------------------------------------------ 5. losses
def _loss_case(cuda, z, iou_type, empty_selection=False):
    """The loss fixture through the kernels: points -> LTRB, both target kernels, the four loss kernels, finalize and all gradients."""
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.modeling.meta_arch.fcos_reppoints import rpd_loss_grads, rpd_loss_sums

    boxes, classes = _load_gts(z)
    K, nl, N = int(z["num_classes"]), len(HW), 2
    sizes = [tuple(int(v) for v in r) for r in z["image_sizes"]]
    lab, reg, ctr, _idx, sel, stats = _assign(cuda, boxes, classes, float(z["radius"]), K=K)
    assert torch.equal(lab.cpu().long(), torch.from_numpy(z["init_gt_classes"])) and torch.equal(sel.cpu().bool(), torch.from_numpy(z["topk_locations"]))
    if empty_selection:
        sel = torch.zeros_like(sel)
        stats = stats.clone()
        stats[1] = 0
    pts = {k: [torch.from_numpy(z[f"{k}{l}"]) for l in range(nl)] for k in ("points_init", "points_refine")}
    init_ltrb, init_boxes, init_arg = _p2l(cuda, _rows(pts["points_init"]))
    refine_ltrb, _b, refine_arg = _p2l(cuda, _rows(pts["points_refine"]), boxes=False)
    _v, _m, _ml, cls, cls_bg, refine_t = _refine(cuda, boxes, classes, init_boxes.cpu(), sizes, K)
    assert torch.equal(cls.cpu().long(), torch.from_numpy(z["refine_gt_classes"])) and torch.equal(refine_t.cpu(), torch.from_numpy(z["refine_reg_targets"]))
    logits = RS.ltrb_rows([torch.from_numpy(z[f"logits{l}"]) for l in range(nl)]).contiguous().to(cuda)
    ctr_logit = RS.ltrb_rows([torch.from_numpy(z[f"ctrness{l}"]) for l in range(nl)]).reshape(N, L).contiguous().to(cuda)
    st = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(HW, STRIDES)]).to(cuda)
    args = (logits, init_ltrb, refine_ltrb, ctr_logit, lab, reg, ctr, sel.to(torch.int32))
    out8, n_ref = rpd_loss_sums(*args, stats, cls, cls_bg, refine_t, st, K, float(z["alpha"]), float(z["gamma"]), iou_type, 1.0)
    g4 = [torch.ones(1, device=cuda) for _ in range(4)]
    dlogits, d_init, d_ref, d_ctr = rpd_loss_grads(g4, out8, n_ref, *args, cls, cls_bg, refine_t, st, K, float(z["alpha"]), float(z["gamma"]), iou_type, 1.0)
    d_pts_init = _p2l_bwd(cuda, d_init.contiguous(), init_arg, N)
    d_pts_ref = _p2l_bwd(cuda, d_ref.contiguous(), refine_arg, N)
    return out8, n_ref, dlogits.view(N, L, -1), d_pts_init, d_pts_ref, d_ctr.view(N, L)


@pytest.mark.parametrize("iou_type", ["giou", "iou"])
def test_losses_equal_the_reference(cuda, iou_type):
    z = np.load(os.path.join(GOLD, f"losses_{iou_type}.npz"))
    nl, K = len(HW), int(z["num_classes"])
    out8, n_ref, dlogits, d_pts_init, d_pts_ref, d_ctr = _loss_case(cuda, z, iou_type)
    assert float(n_ref) == float(z["num_refine_positives"])
    for i, k in enumerate(("cls_loss", "reg_loss_init", "reg_loss", "centerness_loss")):
        a, b = float(out8[i]), float(z["loss::" + k])
        print(k, a, b)
        assert abs(a - b) <= 2e-5 * abs(b), (k, a, b)
    _rel(dlogits[..., :K], RS.ltrb_rows([torch.from_numpy(z[f"grad_logits{l}"]) for l in range(nl)]), 2 ** -7, "d(logits)")
    _rel(d_ctr, RS.ltrb_rows([torch.from_numpy(z[f"grad_ctrness{l}"]) for l in range(nl)]).reshape(2, L), 2 ** -7, "d(centerness)")
    for name, got in (("points_init", d_pts_init), ("points_refine", d_pts_ref)):
        ref = torch.cat([torch.from_numpy(z[f"grad_{name}{l}"]).permute(0, 2, 3, 1).reshape(2, -1, 18) for l in range(nl)], 1)
        have = torch.cat([d32[..., :18].reshape(2, -1, 18) for d32, _ in got], 1)
        _rel(have, ref, 2 ** -7, f"d({name})")


def test_empty_selection_gives_a_zero_init_loss_and_finite_gradients(cuda):
    z = np.load(os.path.join(GOLD, "losses_giou.npz"))
    out8, _n, dlogits, d_pts_init, d_pts_ref, d_ctr = _loss_case(cuda, z, "giou", empty_selection=True)
    assert float(out8[1]) == 0.0 and bool(torch.isfinite(out8).all())
    for t in [dlogits, d_ctr] + [d for d, _ in d_pts_init] + [d for d, _ in d_pts_ref]:
        assert bool(torch.isfinite(t).all())
    assert all(bool((d == 0).all()) for d, _ in d_pts_init) and float(dlogits.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ 6. / 7. the model
@pytest.fixture()
def f32mode():
    from slenderobjdet_amd.layers import functional as HF

    prev = HF.set_precision("fp32")
    yield HF
    HF.set_precision(prev)


# offsets_init's last bias: a 3 x 3 spread of +-8 point strides (= the FPN stride: the init box of a location covers 2 x 2 cells).  At
# random initialisation the nine points coincide, every init box is a point, every IoU ~1e-6 and the matcher's arg-max decisions are
# rounding noise.  (On the CPU oracle this spread gives 23 refine positives for the 18 gt boxes and no IoU within 5e-3 of a threshold.)
SPREAD = [[-8.0, -8.0], [0.0, -8.0], [8.0, -8.0], [-8.0, 0.0], [0.0, 0.0], [8.0, 0.0], [-8.0, 8.0], [0.0, 8.0], [8.0, 8.0]]


def _build(seed=0, spread=True):
    from bench import make_cfg
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.solver import build_optimizer

    cfg = make_cfg(18)
    cfg.MODEL.META_ARCHITECTURE = "FCOSRepPoints"
    torch.manual_seed(seed)
    model = build_model(cfg)
    model.train()
    if spread:
        with torch.no_grad():
            model.head.offsets_init[1].conv.bias[:18] = torch.tensor(SPREAD).reshape(-1).to(model.device)
        model.arena.bump()
    return cfg, model, build_optimizer(cfg, model)


def test_fcos_reppoints_step_in_f32_mode_matches_the_fp32_oracle(cuda, f32mode):
    from slenderobjdet_amd.data import synthetic_batch
    from slenderobjdet_amd.modeling.meta_arch import FCOSRepPoints

    _cfg, model, opt = _build()
    assert type(model) is FCOSRepPoints
    data = synthetic_batch(2, 256, 320, 3, device="cuda")
    cpu = _cpu(data)
    got, masks = _tapped_step(model, opt, data)
    seen = {}

    def make():
        seen["o"] = RS.OracleFCOSRepPoints.from_hip_model(model, emulate_bf16=False)
        return seen["o"]

    def losses_of(o):
        out = o.losses(cpu)
        seen.setdefault("last", []).append(o.last)
        return out

    refs = _forced_oracle_grads(make, losses_of, masks)
    cls, _rt, matches, mlab, vals = (t.cpu() for t in model.last_refine)
    K = model.num_classes
    for last in seen["last"]:            # the fp32 and the float64 oracle
        assert torch.equal(model.last_topk.cpu().bool(), last["sel"]), "selection"
        assert torch.equal(cls.long(), last["cls"]), "refine labels"
        assert torch.equal(matches.long(), last["matches"]), "matches"
    n_gt = sum(len(d["instances"]) for d in data)
    n_pos = int(((cls >= 0) & (cls != K)).sum())
    near = min(float((seen["last"][0]["vals"] - t).abs().min()) for t in model.iou_thresholds)
    print(f"refine positives {n_pos} for {n_gt} gt boxes; smallest |IoU - threshold| {near:.3g}; largest IoU {float(vals.max()):.3f}")
    assert n_pos > n_gt
    for k, b in refs["f32"][0].items():
        a = float(got[k].detach())
        print(k, a, b, refs["f64"][0][k])
        assert abs(a - b) <= 2e-5 * max(abs(b), 1e-3), (k, a, b)
        assert abs(a - refs["f64"][0][k]) <= 2e-5 * max(abs(b), 1e-3), (k, a, refs["f64"][0][k])
    assert sorted(got) == ["centerness_loss", "cls_loss", "reg_loss", "reg_loss_init"]
    _assert_gradients_tight(model, refs, "f32 mode FCOSRepPoints R18")


def test_fcos_reppoints_bf16_step_and_inference(cuda):
    from slenderobjdet_amd.data import synthetic_batch
    from slenderobjdet_amd.layers import functional as HF

    data = synthetic_batch(2, 256, 320, 3, device="cuda")
    prev = HF.set_precision("fp32")
    try:
        _c1, m32, _o1 = _build()
        with torch.no_grad():
            ref = {k: float(v) for k, v in m32(data).items()}
    finally:
        HF.set_precision(prev)
    _c2, model, opt = _build()
    got = model(data)
    opt.zero_grad()
    model.arena.begin_backward(); sum(got.values()).backward(); model.arena.finish_backward()
    opt.step()
    for k, b in ref.items():
        a = float(got[k].detach())
        print(k, a, b)
        assert a == a and abs(a) != float("inf") and abs(a - b) <= 1e-3 * max(abs(b), 1e-3), (k, a, b)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    _c3, m2, _o3 = _build()
    m2.eval()
    m2.pre_nms_thresh = 0.004          # random weights score near PRIOR_PROB = 0.01: let some through
    prev, HF.DETERMINISTIC = HF.DETERMINISTIC, True          # identical GroupNorm statistics in both forwards (float atomics otherwise)
    try:
        with torch.no_grad():
            a, b = m2(data), m2(data)
    finally:
        HF.DETERMINISTIC = prev
    assert sum(len(x["instances"]) for x in a) > 0
    for x, y in zip(a, b):
        x, y = x["instances"], y["instances"]
        assert len(x) == len(y) and torch.equal(x.pred_classes, y.pred_classes)
        assert torch.equal(x.pred_boxes.tensor, y.pred_boxes.tensor) and torch.equal(x.scores, y.scores)
