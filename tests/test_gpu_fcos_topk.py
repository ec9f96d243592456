"""GPU parity of FCOSTopK (slender_det/modeling/meta_arch/fcos/fcos_topk.py): ``sod_fcos_assign_topk`` and the ``sel`` forms of the
regression / centerness loss kernels against the fixtures the reference's own Python produced (tests/golden/fcos_topk/) and against the
restatement (tests/fcos_topk_restated.py, pinned to those fixtures by tests/test_fcos_topk_host.py); the model against the oracle.

Bars: labels, regression targets, gt indices and the selection are exact; centerness targets 1e-6, stats 1e-5 with the count exact
(those of test_gpu_losses.test_fcos_assign); loss sums 2e-5, d(raw) 2^-7 of max|ref| for the bf16 gradient rows, d(scale) 1e-4,
finalize 2e-5 (those of test_gpu_losses.test_fcos_regctr_loss); the fp32-mode step 2e-5 per loss and the 1e-4 / 90 %-within-2e-5
gradient rule of test_gpu_f32_mode; the bf16 step 1e-3 (the README's parity bar)."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fcos_topk_restated as RS
from oracle import fcos_targets as ot
from oracle import losses as ol

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_topk")
HW = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]          # 128 x 160 padded, L = 428
STRIDES = [8, 16, 32, 64, 128]


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


def _assign(cuda, boxes, classes, radius, K=80, topk=5, hw=HW, strides=STRIDES):
    from slenderobjdet_amd.layers import functional as HF

    offs = torch.tensor([0] + [len(b) for b in boxes]).cumsum(0).int()
    if sum(len(b) for b in boxes):
        allb, allc = torch.cat([b.reshape(-1, 4) for b in boxes]).float(), torch.cat(classes).int()
    else:
        allb, allc = torch.zeros(1, 4), torch.zeros(1).int()
    return HF.fcos_assign_topk(allb.to(cuda), allc.to(cuda), offs.to(cuda), len(boxes), hw, strides, ot.SIZES_OF_INTEREST, radius, K, topk)


def _check_against_restatement(cuda, boxes, classes, radius, K=80, topk=5):
    """Kernel == restatement, exactly, on everything discrete; returns the restatement's and the kernel's outputs."""
    ref = RS.topk_targets(HW, STRIDES, boxes, classes, radius, K, topk)
    got = _assign(cuda, boxes, classes, radius, K, topk)
    lab, reg, ctr, idx, sel, stats = (t.cpu() for t in got)
    assert torch.equal(lab.long(), ref[0]), "labels"
    assert torch.equal(reg, ref[1]), "regression targets"
    assert torch.equal(idx.long(), ref[3]), "gt_index"
    assert sel.dtype == torch.uint8 and torch.equal(sel.bool(), ref[4]), "selection"
    _rel(ctr, ref[2], 1e-6, "centerness targets")
    fg = ref[0] != K
    assert float(stats[0]) == float(fg.sum())
    _rel(stats, torch.stack([fg.sum().float(), ref[2][ref[4]].sum(), ref[2].sum()]), 1e-5, "stats3")
    return ref, (lab, reg, ctr, idx, sel, stats)


# ------------------------------------------------------------------------------------------------ 1. targets fixture
@pytest.mark.parametrize("name", ["targets_seed1.npz", "targets_seed2.npz"])
@pytest.mark.parametrize("radius", [1.5, 0.0])
def test_assign_topk_equals_the_reference(cuda, name, radius):
    from slenderobjdet_amd.layers import functional as HF

    z = np.load(os.path.join(GOLD, name))
    boxes, classes = _load_gts(z)
    assert [tuple(int(v) for v in r) for r in z["level_hw"]] == HW
    ref, (lab, reg, ctr, idx, sel, stats) = _check_against_restatement(cuda, boxes, classes, radius)
    assert torch.equal(lab.long(), torch.from_numpy(z[f"gt_classes_r{radius}"]))
    assert torch.equal(reg, torch.from_numpy(z[f"reg_targets_r{radius}"]))
    assert torch.equal(sel.bool(), torch.from_numpy(z[f"topk_locations_r{radius}"]))
    fg = lab != 80
    assert bool((idx[~fg] == -1).all()) and 0 < int(sel.sum()) < int(fg.sum())
    # the first three outputs are those of the plain assignment, bit for bit
    offs = torch.tensor([0] + [len(b) for b in boxes]).cumsum(0).int()
    l2, r2, c2, s2 = HF.fcos_assign(torch.cat(boxes).to(cuda), torch.cat(classes).int().to(cuda), offs.to(cuda), len(boxes), HW, STRIDES,
                                    ot.SIZES_OF_INTEREST, radius, 80)
    assert torch.equal(l2.cpu(), lab) and torch.equal(r2.cpu(), reg) and torch.equal(c2.cpu(), ctr)
    assert float(s2[0]) == float(stats[0])
    _rel(stats[2], s2[1].cpu(), 1e-6, "sum of centerness over the foreground")


# ------------------------------------------------------------------------------------------------ 2. hand-built edge cases
def _t(*rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4)


def _c(*v):
    return torch.tensor(v, dtype=torch.int64)


def test_box_with_no_more_than_k_positives_selects_all(cuda):
    ref, (lab, _r, _c_, _i, sel, _s) = _check_against_restatement(cuda, [_t([10, 10, 24, 22])], [_c(4)], 0.0)
    assert int((lab != 80).sum()) == 4 and int(sel.sum()) == 4


def test_box_between_locations_selects_nothing(cuda):
    ref, (lab, _r, _c_, idx, sel, stats) = _check_against_restatement(cuda, [_t([13, 13, 16, 16], [40, 40, 100, 90])], [_c(4, 5)], 0.0)
    assert not bool((idx == 0).any()) and bool((idx == 1).any()) and int(sel.sum()) == 5


@pytest.mark.parametrize("radius", [0.0, 1.5])
def test_overlapping_boxes_the_smaller_takes_the_shared_locations(cuda, radius):
    ref, (lab, _r, _c_, idx, sel, _s) = _check_against_restatement(cuda, [_t([8.5, 8.5, 72.25, 72.5], [24.25, 24.5, 56.5, 57.0])], [_c(1, 2)], radius)
    inner = idx[0, :320].reshape(16, 20)[4:7, 4:7]
    assert bool((inner == 1).all())
    outer = int((idx[0] == 0).sum())          # radius 1.5: the outer box's centre region lies inside the inner box, nothing is left of it
    assert outer > 5 if radius == 0 else outer == 0
    assert int(sel[0][idx[0] == 0].sum()) == min(outer, 5) and int(sel[0][idx[0] == 1].sum()) == 5


def test_second_of_two_identical_boxes_selects_nothing(cuda):
    ref, (lab, _r, _c_, idx, sel, _s) = _check_against_restatement(cuda, [_t([20.5, 18.25, 90.0, 70.5], [20.5, 18.25, 90.0, 70.5])], [_c(1, 2)], 0.0)
    assert not bool((idx == 1).any()) and int(sel.sum()) == 5 and bool((lab[sel.bool()] == 1).all())


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


def test_box_covering_the_whole_coarsest_level(cuda):
    ref, (lab, _r, _c_, idx, sel, _s) = _check_against_restatement(cuda, [_t([-600.0, -600.0, 800.0, 700.0], [30.25, 20.5, 140.0, 100.5])], [_c(1, 2)], 0.0)
    assert (lab[0, -2:] == 1).all() and int(sel[0, -2:].sum()) == 2


@pytest.mark.parametrize("topk", [1, 8])
def test_other_k(cuda, topk):
    z = np.load(os.path.join(GOLD, "targets_seed1.npz"))
    boxes, classes = _load_gts(z)
    ref, (lab, _r, _c_, idx, sel, _s) = _check_against_restatement(cuda, boxes, classes, 0.0, topk=topk)
    per_gt = [int(sel[idx == g].sum()) for g in range(sum(len(b) for b in boxes))]
    assert max(per_gt) == topk


def test_tie_at_the_cut_takes_the_lower_location(cuda):
    """Box (8, 8, 40, 40), radius 0: centerness 4 x 0.6, 8 x 0.2928, 4 x 0.1429 on the stride-8 level.  The four 0.6 and the lowest-index
    0.2928 (the CPU reference's torch.topk happens to pick another one: checked against the restatement only)."""
    ref, (lab, _r, ctr, _i, sel, _s) = _check_against_restatement(cuda, [_t([8, 8, 40, 40])], [_c(3)], 0.0)
    pos = (lab[0] != 80).nonzero().squeeze(1)
    vals = ctr[0, pos]
    assert pos.numel() == 16 and int((vals > 0.5).sum()) == 4
    mid = pos[(vals > 0.2) & (vals < 0.5)]
    assert mid.numel() == 8 and len(set(vals[(vals > 0.2) & (vals < 0.5)].tolist())) == 1          # an exact eight-way tie on the device
    assert set(sel[0].nonzero().squeeze(1).tolist()) == set(pos[vals > 0.5].tolist()) | {int(mid.min())}


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


# ------------------------------------------------------------------------------------------------ 3. loss kernels
def _run_loss_kernels(cuda, raw, scales, targets, K, loss_type, norm_reg, sel, g_reg=1.0, g_ctr=1.0, stats=None):
    """The sel (or, with sel None, the plain) forward / backward / finalize on raw (M, 8): columns 0..3 box, 4 centerness logit."""
    from slenderobjdet_amd.layers import functional as HF

    lab, reg, ctr = targets
    N, M = lab.shape[0], raw.shape[0]
    raw_d = raw.to(cuda)
    sc = scales.to(cuda)
    sums = HF.fcos_regctr_loss_fwd(raw_d, 8, raw_d.view(-1)[4:], 8, lab, reg, ctr, sc, N, HW, STRIDES, K, loss_type, norm_reg, sel=sel)
    dbox = torch.full((M, 8), 9.0, dtype=torch.bfloat16, device=cuda)
    dsc = torch.zeros(5, device=cuda)
    HF.fcos_regctr_loss_bwd(raw_d, 8, raw_d.view(-1)[4:], 8, lab, reg, ctr, sc, N, HW, STRIDES, K, loss_type, norm_reg,
                            torch.tensor([g_reg], device=cuda), torch.tensor([g_ctr], device=cuda), stats, 1.0, dbox, 8, 4, dbox, 8, 4, dsc, sel=sel)
    return sums, dbox, dsc


@pytest.mark.parametrize("loss_type", ["giou", "iou"])
def test_sel_loss_kernels_equal_the_reference(cuda, loss_type):
    """The reference's losses take final box predictions: raw = log(pred) with unit scales gives them back through the kernel's exp, and
    d(raw) = d(pred) * pred."""
    from slenderobjdet_amd.layers import functional as HF

    z = np.load(os.path.join(GOLD, f"losses_{loss_type}.npz"))
    boxes, classes = _load_gts(z)
    K, nl = int(z["num_classes"]), len(HW)
    lab, reg, ctr, _idx, sel, stats = _assign(cuda, boxes, classes, float(z["radius"]), K=K)
    assert torch.equal(lab.cpu().long(), torch.from_numpy(z["gt_classes"])) and torch.equal(sel.cpu().bool(), torch.from_numpy(z["topk_locations"]))
    pl = [[torch.from_numpy(z[f"{k}{l}"]) for l in range(nl)] for k in ("logits", "box_reg", "ctrness")]
    gl = [[torch.from_numpy(z[f"grad_{k}{l}"]) for l in range(nl)] for k in ("logits", "box_reg", "ctrness")]
    cls, box, cts = RS.permute_and_concat(pl[0], pl[1], pl[2], K)
    gcls, gbox, gcts = RS.permute_and_concat(gl[0], gl[1], gl[2], K)
    raw = torch.zeros(box.shape[0], 8)
    raw[:, :4], raw[:, 4] = torch.log(box), cts
    sums, dbox, dsc = _run_loss_kernels(cuda, raw, torch.ones(5), (lab, reg, ctr), K, loss_type, False, sel, stats=stats)
    focal_sum, _ = HF.focal_loss_fwd(cls.contiguous().to(cuda), lab.reshape(-1), None, float(z["alpha"]), float(z["gamma"]), K=K)
    out3 = HF.fcos_finalize_losses(focal_sum, sums, stats, 1.0)
    ref3 = torch.tensor([float(z["loss::cls_loss"]), float(z["loss::reg_loss"]), float(z["loss::centerness_loss"])])
    _rel(out3, ref3, 2e-5, "finalize")
    for i in range(3):
        assert abs(float(out3[i]) - float(ref3[i])) <= 2e-5 * abs(float(ref3[i])), (i, float(out3[i]), float(ref3[i]))
    _rel(dbox[:, :4], gbox * box, 2 ** -7, "d(raw box)")
    _rel(dbox[:, 4], gcts, 2 ** -7, "d(centerness logit)")
    assert (dbox[:, 5:] == 0).all()


def test_sel_loss_kernels_linear_iou_norm_reg_vs_restatement(cuda):
    z = np.load(os.path.join(GOLD, "targets_seed1.npz"))
    boxes, classes = _load_gts(z)
    N, L = len(boxes), sum(h * w for h, w in HW)
    labels, reg_t, _ctr, _idx, sel = RS.topk_targets(HW, STRIDES, boxes, classes, 1.5, 80)
    g = torch.Generator().manual_seed(0)
    raw = torch.randn(N * L, 8, generator=g) * 0.5 + 0.2
    raw[:, :4] += 0.6                                                     # relu(z) * stride: most predictions positive, some clipped
    scales = torch.tensor([1.0, 0.9, 1.1, 1.2, 0.8])
    lvl_of = torch.cat([torch.full((h * w,), i) for i, (h, w) in enumerate(HW)]).repeat(N)
    st_of = torch.tensor(STRIDES, dtype=torch.float32)[lvl_of]
    rawr, sc = raw.clone().requires_grad_(True), scales.clone().requires_grad_(True)
    pred = torch.relu(rawr[:, :4] * sc[lvl_of][:, None]) * st_of[:, None]
    lab, rt, sl = labels.reshape(-1), reg_t.reshape(-1, 4), sel.reshape(-1)
    fg = lab != 80
    ctr_fg, ctr_sel = ol.centerness_targets(rt[fg]), ol.centerness_targets(rt[sl])
    reg_sum = ol.iou_loss_ltrb(pred[sl], rt[sl], ctr_sel, "linear_iou")
    ctr_sum = F.binary_cross_entropy_with_logits(rawr[:, 4][fg], ctr_fg, reduction="sum")
    npos, ssel = float(fg.sum()), float(ctr_sel.sum())
    graw, gsc = torch.autograd.grad(reg_sum / ssel * 0.7 + ctr_sum / max(npos, 1.0) * 1.3, (rawr, sc))

    from slenderobjdet_amd.layers import functional as HF
    hl, hr, hc, _i, hs, stats = _assign(cuda, boxes, classes, 1.5)
    assert torch.equal(hs.cpu().bool(), sel)
    sums, dbox, dsc = _run_loss_kernels(cuda, raw, scales, (hl, hr, hc), 80, "linear_iou", True, hs, 0.7, 1.3, stats)
    _rel(sums, torch.stack([reg_sum, ctr_sum]), 2e-5, "regctr sums")
    _rel(dbox[:, :5], graw[:, :5], 2 ** -7, "regctr d(raw)")
    assert (dbox[:, 5:] == 0).all()
    _rel(dsc, gsc, 1e-4, "d(scale)")
    out3 = HF.fcos_finalize_losses(torch.tensor([5.0], device=cuda), sums, stats, 1.0)
    _rel(out3, torch.stack([torch.tensor(5.0 / max(npos, 1)), reg_sum / ssel, ctr_sum / max(npos, 1)]), 2e-5, "finalize")
    # rows outside the selection: exactly zero box gradient, centerness gradient as ever
    out = (fg & ~sl).to(cuda)
    assert int(out.sum()) > 0 and bool((dbox[out][:, :4] == 0).all()) and bool((dbox[out][:, 4] != 0).all())


@pytest.mark.parametrize("loss_type,norm_reg", [("giou", False), ("linear_iou", True)])
def test_sel_of_all_foreground_is_the_existing_kernel_bit_for_bit(cuda, loss_type, norm_reg):
    from slenderobjdet_amd.layers import functional as HF

    z = np.load(os.path.join(GOLD, "targets_seed2.npz"))
    boxes, classes = _load_gts(z)
    N, L = len(boxes), sum(h * w for h, w in HW)
    offs = torch.tensor([0] + [len(b) for b in boxes]).cumsum(0).int()
    lab, reg, ctr, stats = HF.fcos_assign(torch.cat(boxes).to(cuda), torch.cat(classes).int().to(cuda), offs.to(cuda), N, HW, STRIDES,
                                          ot.SIZES_OF_INTEREST, 1.5, 80)
    raw = torch.randn(N * L, 8, generator=torch.Generator().manual_seed(1)) * 0.5 + (0.5 if norm_reg else 1.0)
    scales = torch.tensor([1.0, 0.9, 1.1, 1.2, 0.8])
    all_fg = (lab != 80).to(torch.uint8).contiguous()
    a = _run_loss_kernels(cuda, raw, scales, (lab, reg, ctr), 80, loss_type, norm_reg, None, 0.7, 1.3, stats)
    b = _run_loss_kernels(cuda, raw, scales, (lab, reg, ctr), 80, loss_type, norm_reg, all_fg, 0.7, 1.3, stats)
    for x, y, what in zip(a, b, ("sums", "d(raw)", "d(scale)")):
        assert torch.equal(x, y), what
    assert float(a[0][0]) != 0 and float(a[2].abs().sum()) != 0


# ------------------------------------------------------------------------------------------------ 4. / 5. the model
@pytest.fixture()
def f32mode():
    from slenderobjdet_amd.layers import functional as HF

    prev = HF.set_precision("fp32")
    yield HF
    HF.set_precision(prev)


@contextlib.contextmanager
def _forced(masks):
    """The oracle code inside takes the PRODUCT's ReLU decisions (oracle.nn.ForcedMasks) wherever ``masks`` has the position; the two may
    differ only where a pre-activation is zero to rounding."""
    from oracle.nn import ForcedMasks

    st = ForcedMasks.begin(masks)
    try:
        yield st
    finally:
        ForcedMasks.end()
    assert st["outside"] == 0, ("ReLU decisions differ outside the undecided band", st["outside_at"][:5])


def _tapped_step(model, opt, data):
    from oracle.conditioning import ProductReluTap

    with ProductReluTap() as tap:
        got = model(data)
        opt.zero_grad()
        model.arena.begin_backward(); sum(got.values()).backward(); model.arena.finish_backward()
    masks, unmatched = tap.masks_for(model)
    assert not unmatched, unmatched[:5]
    return got, masks


def _forced_oracle_grads(make_oracle, losses_of, masks):
    refs = {}
    for tag in ("f32", "f64"):
        oracle = make_oracle()
        if tag == "f64":
            oracle.double()
        with _forced(masks) as st:
            losses = losses_of(oracle)
            tr = oracle.trainable()
            grads = dict(zip(tr.keys(), torch.autograd.grad(sum(losses.values()), list(tr.values()), allow_unused=True)))
        assert not st["missed"], st["missed"][:5]
        refs[tag] = ({k: float(v.detach()) for k, v in losses.items()}, grads)
    return refs


def _assert_gradients_tight(model, refs, what, max_pair=1e-4, share_2e5=0.9):
    """Every parameter gradient within 1e-4 of its norm from the fp32 and the float64 oracle, 90 % of the tensors within 2e-5."""
    rows = []
    for name, p in model.named_parameters():
        if not p.requires_grad or refs["f64"][1].get(name) is None:
            continue
        gq = p.grad.detach().double().cpu()
        if gq.dim() == 4:
            gq = gq.permute(0, 3, 1, 2)
        r64, r32 = refs["f64"][1][name], refs["f32"][1][name].double()
        if gq.shape != r64.shape:          # padded prediction rows beyond the reference's
            assert gq.shape[1:] == r64.shape[1:] and (gq[r64.shape[0]:] == 0).all(), (name, gq.shape, r64.shape)
            gq = gq[: r64.shape[0]]
        n = max(r64.norm().item(), 1e-30)
        rows.append(((gq - r32).norm().item() / n, (gq - r64).norm().item() / n, name))
    assert len(rows) >= 20, len(rows)
    share = sum(r[0] <= 2e-5 and r[1] <= 2e-5 for r in rows) / len(rows)
    print(f"\n{what}: {len(rows)} tensors, worst hip32-cpu32 {max(rows)[0]:.2e} ({max(rows)[2]}), worst hip32-f64 {max(r[1] for r in rows):.2e}, share <= 2e-5: {share:.3f}")
    for d32, d64, name in rows:
        assert d32 <= max_pair and d64 <= max_pair, (what, name, d32, d64)
    assert share >= share_2e5, (what, share, sorted(rows)[-5:])


def _build(arch, seed=0, box_bias=None):
    """``box_bias``: bias of the four box channels.  At the initial 0 every prediction is exp(~0) = 1 px, every GIoU loss is ~1 and the
    regression loss is ~1 whichever rows it averages over; exp(3) = 20 px makes it depend on the rows."""
    from bench import make_cfg
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.solver import build_optimizer

    cfg = make_cfg(18)
    cfg.MODEL.META_ARCHITECTURE = arch
    torch.manual_seed(seed)
    model = build_model(cfg)
    model.train()
    if box_bias is not None:
        with torch.no_grad():
            model.head.box_pred.bias[:4].fill_(box_bias)
        model.arena.bump()
    return cfg, model, build_optimizer(cfg, model)


def _cpu(data):
    return [{"image": d["image"].cpu(), "instances": d["instances"].to("cpu")} for d in data]


def test_fcos_topk_step_in_f32_mode_matches_the_fp32_oracle(cuda, f32mode):
    from slenderobjdet_amd.data import synthetic_batch
    from slenderobjdet_amd.modeling.meta_arch import FCOSTopK

    _cfg, model, opt = _build("FCOSTopK", box_bias=3.0)
    assert type(model) is FCOSTopK
    data = synthetic_batch(2, 256, 320, 3, device="cuda")
    cpu = _cpu(data)
    got, masks = _tapped_step(model, opt, data)
    seen = {}

    def make():
        seen["o"] = RS.OracleFCOSTopK.from_hip_model(model, emulate_bf16=False)
        return seen["o"]

    refs = _forced_oracle_grads(make, lambda o: o.losses(cpu), masks)
    sel = model.last_topk.cpu().bool()
    assert torch.equal(sel, seen["o"].last_sel)
    for k, b in refs["f32"][0].items():
        a = float(got[k].detach())
        print(k, a, b, refs["f64"][0][k])
        assert abs(a - b) <= 2e-5 * max(abs(b), 1e-3), (k, a, b)
        assert abs(a - refs["f64"][0][k]) <= 2e-5 * max(abs(b), 1e-3), (k, a, refs["f64"][0][k])
    _assert_gradients_tight(model, refs, "f32 mode FCOSTopK R18")
    # classification and centerness keep all positives: those two losses are an FCOS model's; the regression loss is not
    _c2, fcos, _o2 = _build("FCOS", box_bias=3.0)
    ref = fcos(data)
    for k in ("cls_loss", "centerness_loss"):
        a, b = float(got[k].detach()), float(ref[k].detach())
        assert abs(a - b) <= 2e-5 * max(abs(b), 1e-3), (k, a, b)
    a, b = float(got["reg_loss"].detach()), float(ref["reg_loss"].detach())
    assert abs(a - b) > 1e-4 * abs(b), (a, b)       # more than the two 2e-5 bars above can account for
    assert 0 < int(sel.sum()) < int((seen["o"].last_labels != 80).sum())


def test_fcos_topk_bf16_step_and_inference(cuda):
    from slenderobjdet_amd.data import synthetic_batch
    from slenderobjdet_amd.layers import functional as HF

    data = synthetic_batch(2, 256, 320, 3, device="cuda")
    prev = HF.set_precision("fp32")
    try:
        _c1, m32, _o1 = _build("FCOSTopK")
        with torch.no_grad():
            ref = {k: float(v) for k, v in m32(data).items()}
    finally:
        HF.set_precision(prev)
    _c2, model, opt = _build("FCOSTopK")
    got = model(data)
    opt.zero_grad()
    model.arena.begin_backward(); sum(got.values()).backward(); model.arena.finish_backward()
    opt.step()
    for k, b in ref.items():
        a = float(got[k].detach())
        print(k, a, b)
        assert a == a and abs(a) != float("inf") and abs(a - b) <= 1e-3 * max(abs(b), 1e-3), (k, a, b)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    # inference is FCOSV2's: same weights (same seed), same detections
    _c3, m2, _o3 = _build("FCOSTopK")
    _c4, v2, _o4 = _build("FCOSV2")
    for m in (m2, v2):
        m.eval()
        m.pre_nms_thresh = 0.004          # random weights score near PRIOR_PROB = 0.01: let some through
    prev, HF.DETERMINISTIC = HF.DETERMINISTIC, True          # identical GroupNorm statistics in both forwards (float atomics otherwise)
    try:
        with torch.no_grad():
            a, b = m2(data), v2(data)
    finally:
        HF.DETERMINISTIC = prev
    assert sum(len(x["instances"]) for x in a) > 0
    for x, y in zip(a, b):
        x, y = x["instances"], y["instances"]
        assert len(x) == len(y) and torch.equal(x.pred_classes, y.pred_classes)
        assert torch.equal(x.pred_boxes.tensor, y.pred_boxes.tensor) and torch.equal(x.scores, y.scores)


# ------------------------------------------------------------------------------------------------ 6. cross-check
def test_selection_equals_lrtb_topk_head(cuda):
    """On a batch without duplicate boxes or ties at the cut (checked), the kernel's selection is the mask LRTBTopkHead.init_selection's
    host loop leaves in ``last_topk`` (same targets, same centerness values, same k)."""
    from bench import make_cfg
    from slenderobjdet_amd.data import synthetic_batch
    from slenderobjdet_amd.modeling import build_model

    cfg = make_cfg(18)
    cfg.MODEL.META_ARCHITECTURE = "AblationMetaArch"
    cfg.MODEL.BACKBONE.NAME = "build_retinanet_resnet_fpn_backbone"
    m = cfg.MODEL.META_ARCH
    m.NAME, m.NUM_POINTS, m.FEAT_ADAPTION, m.RES_REFINE = "LRTBTopkHead", 2, "Empty", False
    m.NORM_REG_TARGETS, m.CENTERNESS_ON_LOC, m.IOU_LOSS_TYPE, m.SLENDER_CENTERNESS, m.CENTER_SAMPLING_RADIUS = True, True, "giou", False, 0.0
    torch.manual_seed(12)
    model = build_model(cfg)
    model.train()
    data = synthetic_batch(2, 192, 256, 16, device="cuda")
    # the synthetic boxes are clipped to the image: one spanning its whole height is centred on a row of locations and ties in pairs.
    # Shrink every side by a random fraction of a few pixels (sides are >= 16 px) so that no two positives of a box are mirror images
    g = torch.Generator().manual_seed(5)
    for d in data:
        b = d["instances"].gt_boxes.tensor
        b += ((torch.rand(b.shape, generator=g) * 2.8 + 0.1) * torch.tensor([1.0, 1.0, -1.0, -1.0])).to(b.device)
    model(data)
    head = model.head
    mine = head.last_topk.cpu()
    hw = [(24, 32), (12, 16), (6, 8), (3, 4), (2, 2)]
    gtb = [d["instances"].gt_boxes.tensor.cpu() for d in data]
    gtc = [d["instances"].gt_classes.cpu() for d in data]
    assert tuple(mine.shape) == (2, sum(h * w for h, w in hw))
    # preconditions, on the restatement: no duplicate boxes, and the 5th / 6th centerness of every gt apart by more than rounding
    lab, reg, ctr, idx, _sel = RS.topk_targets(hw, head.fpn_strides, gtb, gtc, 0.0, 80)
    for b in gtb:
        assert torch.unique(b, dim=0).shape[0] == b.shape[0]
    for g in range(sum(len(b) for b in gtb)):
        s = ctr[idx == g].sort(descending=True).values
        assert s.numel() <= 5 or float(s[4] - s[5]) > 1e-5 * float(s[4]), (g, s[:7])
    offs = torch.tensor([0] + [len(b) for b in gtb]).cumsum(0).int()
    from slenderobjdet_amd.layers import functional as HF
    out = HF.fcos_assign_topk(torch.cat(gtb).to(cuda), torch.cat(gtc).int().to(cuda), offs.to(cuda), 2, hw, head.fpn_strides,
                              ot.SIZES_OF_INTEREST, 0.0, 80, head.topk_per_box)
    assert torch.equal(out[0].cpu(), head.last_targets[0].cpu())
    assert int(mine.sum()) > 5 and torch.equal(out[4].cpu().bool(), mine)
