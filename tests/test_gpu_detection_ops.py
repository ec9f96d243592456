"""GPU parity for the detection operators: NMS keep indices bit-exact (north_star), ROIAlign / box losses to 1e-5 relative,
anchor labels bit-exact.  Adversarial cases: score ties, touching boxes, zero-area boxes, empty inputs."""
import pytest
import torch

from oracle import detection as od
from oracle import losses as ol

pytestmark = pytest.mark.gpu


def _g(s):
    return torch.Generator().manual_seed(s)


def _boxes(n, seed, size=200.0):
    g = _g(seed)
    xy = torch.rand(n, 2, generator=g) * size
    wh = torch.rand(n, 2, generator=g) * 60 + 1
    return torch.cat([xy, xy + wh], 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 500, 3000])
@pytest.mark.parametrize("thr", [0.5, 0.6])
def test_nms_keep_indices_bit_exact(cuda, n, thr):
    from slenderobjdet_amd.layers import functional as HF

    b = _boxes(n, n)
    s = torch.rand(n, generator=_g(n + 1))
    if n > 10:
        s[5] = s[3]                      # score tie: stable order decides
        b[7] = b[2]                      # identical boxes (IoU == 1)
        b[9] = torch.tensor([10.0, 10.0, 10.0, 30.0])   # zero-area box (IoU 0/0 = NaN -> never suppresses)
        b[11, :2] = b[4, 2:]             # touching corner: IoU == 0
    keep = HF.nms(b.to(cuda), s.to(cuda), thr)
    assert torch.equal(keep.cpu(), od.nms(b, s, thr))


def test_batched_nms_and_empty(cuda):
    from slenderobjdet_amd.layers.nms import batched_nms

    b, s = _boxes(800, 3), torch.rand(800, generator=_g(4))
    idx = torch.randint(0, 80, (800,), generator=_g(5))
    assert torch.equal(batched_nms(b.to(cuda), s.to(cuda), idx.to(cuda), 0.6).cpu(), od.batched_nms(b, s, idx, 0.6))
    assert batched_nms(b[:0].to(cuda), s[:0].to(cuda), idx[:0].to(cuda), 0.6).numel() == 0


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("sampling_ratio", [0, 2])
def test_roi_align_fwd_bwd(cuda, rotated, sampling_ratio):
    from oracle import nn as onn
    from slenderobjdet_amd.layers import functional as HF

    N, C, H, W = 2, 16, 20, 24
    x = onn.rb(torch.randn(N, C, H, W, generator=_g(0)))
    if rotated:
        rois = torch.tensor([[0, 40.0, 36.0, 50.0, 30.0, 30.0], [1, 60.0, 40.0, 20.0, 70.0, -75.0], [0, 5.0, 5.0, 30.0, 12.0, 0.0], [1, 90.0, 70.0, 40.0, 40.0, 45.0]])
    else:
        rois = torch.tensor([[0, 8.0, 6.0, 70.0, 60.0], [1, 0.0, 0.0, 95.0, 79.0], [0, 30.5, 20.25, 33.0, 28.0], [1, -10.0, -5.0, 20.0, 30.0], [0, 90.0, 70.0, 120.0, 100.0]])
    xr = x.clone().requires_grad_(True)
    ref = od.roi_align(xr, rois, (7, 7), 0.25, sampling_ratio, rotated)
    out = HF.roi_align_fwd(x.permute(0, 2, 3, 1).contiguous().to(cuda).bfloat16(), rois.to(cuda), (7, 7), 0.25, sampling_ratio, rotated)
    err = (out.cpu().permute(0, 3, 1, 2) - ref.detach()).abs().max().item()
    assert err <= 1e-5 * max(ref.abs().max().item(), 1.0), err
    dout = torch.randn(ref.shape, generator=_g(1))
    (gref,) = torch.autograd.grad(ref, xr, dout)
    dx = HF.roi_align_bwd(dout.permute(0, 2, 3, 1).contiguous().to(cuda), rois.to(cuda), (N, H, W, C), 0.25, sampling_ratio, rotated)
    err = (dx.cpu().permute(0, 3, 1, 2) - gref).abs().max().item()
    assert err <= 2e-5 * max(gref.abs().max().item(), 1.0), err


def test_giou_and_smooth_l1(cuda):
    from slenderobjdet_amd.layers import functional as HF

    b1, b2 = _boxes(400, 1), _boxes(400, 2)
    b1[3] = b2[3]
    b1[5] = torch.tensor([0.0, 0.0, 5.0, 5.0]); b2[5] = torch.tensor([50.0, 50.0, 60.0, 60.0])   # disjoint
    br = b1.clone().requires_grad_(True)
    ref = ol.giou_loss_xyxy(br, b2)
    (gref,) = torch.autograd.grad(ref.sum() * 0.3, br)
    elem, s, d1 = HF.giou_loss_xyxy(b1.to(cuda), b2.to(cuda), want_grad=True, grad_scale=torch.tensor([0.3], device=cuda))
    assert (elem.cpu() - ref.detach()).abs().max() < 1e-5 and abs(s.item() - ref.sum().item()) < 1e-3
    assert (d1.cpu() - gref).abs().max() < 1e-5
    x, t = torch.randn(1000, generator=_g(3)), torch.randn(1000, generator=_g(4))
    for beta in (0.11, 0.0):
        xr = x.clone().requires_grad_(True)
        ref = ol.smooth_l1_loss(xr, t, beta)
        (gref,) = torch.autograd.grad(ref.sum(), xr)
        elem, s, dx = HF.smooth_l1_loss(x.to(cuda), t.to(cuda), beta, want_grad=True)
        assert (elem.cpu() - ref.detach()).abs().max() < 1e-6 and (dx.cpu() - gref).abs().max() < 1e-6


@pytest.mark.parametrize("G", [0, 1, 7, 40])
def test_anchor_match_bit_exact(cuda, G):
    from slenderobjdet_amd.layers import functional as HF

    anchors = _boxes(5000, 9, 300.0)
    gts = _boxes(G, 10, 300.0) if G else torch.zeros(0, 4)
    if G > 2:
        anchors[17] = gts[1]          # exact match (IoU 1)
        gts[2] = torch.tensor([1000.0, 1000.0, 1010.0, 1010.0])   # gt overlapping no anchor: detectron2 promotes every IoU==0 anchor
    q = od.pairwise_iou(gts, anchors) if G else torch.zeros(0, 5000)
    m_ref, l_ref = od.matcher(q, [0.4, 0.5], [0, -1, 1], True)
    vals, idx, lab = HF.anchor_match(gts.to(cuda), anchors.to(cuda), [0.4, 0.5], [0, -1, 1], True)
    assert torch.equal(lab.cpu(), l_ref)
    if G:
        assert torch.equal(idx.cpu().long(), m_ref)
        assert torch.equal(vals.cpu(), q.max(dim=0).values)


def _rboxes(n, seed):
    g = _g(seed)
    c = torch.rand(n, 2, generator=g) * 120
    wh = torch.rand(n, 2, generator=g) * 50 + 2
    ang = (torch.rand(n, 1, generator=g) - 0.5) * 180
    return torch.cat([c, wh, ang], 1)


def test_box_iou_rotated_known_values_and_oracle(cuda):
    from slenderobjdet_amd.layers import functional as HF

    b1 = torch.tensor([[50.0, 50.0, 20.0, 10.0, 0.0], [50.0, 50.0, 20.0, 10.0, 0.0], [0.0, 0.0, 2.0, 2.0, 0.0], [10.0, 10.0, 4.0, 4.0, 45.0]])
    b2 = torch.tensor([[50.0, 50.0, 20.0, 10.0, 0.0], [50.0, 50.0, 10.0, 20.0, 90.0], [1.0, 0.0, 2.0, 2.0, 0.0], [100.0, 100.0, 4.0, 4.0, 0.0]])
    got = HF.box_iou_rotated(b1.to(cuda), b2.to(cuda)).cpu()
    assert abs(got[0, 0] - 1.0) < 1e-5 and abs(got[1, 1] - 1.0) < 1e-4      # same box; same box described with w/h swapped + 90 deg
    assert abs(got[2, 2] - 1.0 / 3.0) < 1e-5 and got[3, 3] == 0
    r1, r2 = _rboxes(40, 1), _rboxes(50, 2)
    ref = od.pairwise_iou_rotated(r1, r2)
    got = HF.box_iou_rotated(r1.to(cuda), r2.to(cuda)).cpu()
    assert (got - ref).abs().max() < 2e-4        # fp32 sin/cos and clipping order differ in the last ulps


def _rboxes_clustered(n, seed):
    """Jittered copies of 8 slender boxes, all centres inside a 60 x 60 px square: every 64 x 64 block of pairs holds far more than
    64 pairs that pass the circle test, and many of them overlap above any threshold."""
    g = _g(seed)
    proto = torch.cat([300 + 8 + torch.rand(8, 2, generator=g) * 44, torch.rand(8, 1, generator=g) * 30 + 30, torch.rand(8, 1, generator=g) * 12 + 8,
                       (torch.rand(8, 1, generator=g) - 0.5) * 180], 1)
    b = proto[torch.arange(n) % 8]
    b[:, :2] += (torch.rand(n, 2, generator=g) - 0.5) * 8
    b[:, 2:4] *= 0.85 + torch.rand(n, 2, generator=g) * 0.3
    b[:, 4] += (torch.rand(n, generator=g) - 0.5) * 12
    b[[20, 90, 150], 3] = torch.tensor([0.5, 0.9, 0.25])      # a side below 1 px: these pairs bypass the prefilter
    return b


@pytest.mark.parametrize("thr", [0.3, 0.5, 0.7])
@pytest.mark.parametrize("boxset", ["spread", "clustered"])
def test_nms_rotated_keep_indices(cuda, boxset, thr):
    """Greedy rotated NMS: keep indices bit-exact w.r.t. the oracle's greedy scan over the SAME IoU matrix (the IoU values
    themselves are checked against the oracle above to 2e-4; with 90k pairs some always sit within float noise of any threshold).
    The clustered set (seed 3: the CPU oracle's greedy scan keeps 15 / 25 / 67 of its 200 boxes at 0.3 / 0.5 / 0.7) sends far more
    than 64 pairs of one block through the prefilter and the compaction of the mask kernel."""
    import numpy as np

    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.layers.nms import batched_nms_rotated

    def greedy(iou, scores, thr):
        order = torch.sort(scores, descending=True, stable=True).indices.numpy()
        keep, dead = [], np.zeros(len(scores), dtype=bool)
        for pos, i in enumerate(order):
            if dead[i]:
                continue
            keep.append(int(i))
            rest = order[pos + 1:]
            dead[rest[iou[i, rest] > np.float32(thr)]] = True
        return torch.tensor(keep, dtype=torch.int64)

    if boxset == "spread":
        b, s = _rboxes(300, 3), torch.rand(300, generator=_g(4))
    else:
        b, s = _rboxes_clustered(200, 3), torch.rand(200, generator=_g(4))
    b[5] = b[2]
    s[9] = s[4]
    iou = HF.box_iou_rotated(b.to(cuda), b.to(cuda)).cpu().numpy()
    assert torch.equal(HF.nms_rotated(b.to(cuda), s.to(cuda), thr).cpu(), greedy(iou, s, thr))
    if boxset != "spread" or thr != 0.5:
        return
    idx = torch.randint(0, 3, (300,), generator=_g(5))
    keep = batched_nms_rotated(b.to(cuda), s.to(cuda), idx.to(cuda), 0.5).cpu()
    ref = []
    for c in range(3):
        sel = torch.nonzero(idx == c).squeeze(1)
        ref += sel[greedy(iou[np.ix_(sel.numpy(), sel.numpy())], s[sel], 0.5)].tolist()
    # class offsets shift the centres by thousands of pixels, which perturbs the clipped polygon in the last float digits:
    # allow a pair sitting exactly at the threshold to flip
    assert len(set(keep.tolist()) ^ set(ref)) <= 2


@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("box_dim", [4, 5])
def test_nms_single_equals_batched_of_one(cuda, box_dim, n):
    """The single-image calls run the batched kernels with B = 1; class 0 shifts nothing, so both see bit-identical boxes."""
    from slenderobjdet_amd.layers import functional as HF

    b = (_boxes(n, n) if box_dim == 4 else _rboxes(n, n)).to(cuda)
    s = torch.rand(n, generator=_g(n + 1)).to(cuda)
    single = (HF.nms if box_dim == 4 else HF.nms_rotated)(b, s, 0.5)
    keep, nkeep = HF.batched_nms_topk(b[None].contiguous(), s[None].contiguous(), torch.zeros((1, n), dtype=torch.int32, device=cuda), 0.5, n)
    assert torch.equal(keep[0, : int(nkeep[0])], single)


def test_anchor_match_full_size_bit_exact(cuda):
    """BASELINE configs[2] size: A = 201 600 anchors (800x1344, 9 per location), G up to 50: labels, matched indices and matched
    IoUs bit-exact vs the oracle's explicit G x A matrix + detectron2 Matcher (retina_rotated.py:251-295), including the
    low-quality pass.  Property on top: every gt whose best IoU is > 0 owns at least one positive anchor."""
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.modeling.anchor_generator import grid_anchors

    hw = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
    sizes = [[x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)] for x in [32, 64, 128, 256, 512]]
    anchors = torch.cat(grid_anchors(hw, [8, 16, 32, 64, 128], sizes, [[0.5, 1.0, 2.0]] * 5))
    assert anchors.shape[0] == 201600
    ad = anchors.to(cuda)
    for G, seed in ((1, 3), (7, 4), (50, 5)):
        g = _g(seed)
        c = torch.rand(G, 2, generator=g) * torch.tensor([1333.0, 800.0])
        wh = torch.pow(2.0, torch.rand(G, 2, generator=g) * 5.2 + 4.0)
        gts = torch.cat([(c - wh / 2).clamp(min=0), torch.minimum(c + wh / 2, torch.tensor([1333.0, 800.0]))], 1)
        q = od.pairwise_iou(gts, anchors)
        m_ref, l_ref = od.matcher(q, [0.4, 0.5], [0, -1, 1], True)
        vals, idx, lab = HF.anchor_match(gts.to(cuda), ad, [0.4, 0.5], [0, -1, 1], True)
        assert torch.equal(lab.cpu(), l_ref) and torch.equal(idx.cpu().long(), m_ref) and torch.equal(vals.cpu(), q.max(dim=0).values), G
        best = q.max(dim=1).values
        for j in range(G):
            if best[j] > 0:
                assert ((l_ref == 1) & (q[j] == best[j])).any()


# ---------------------------------------------------------------------------------------------- the five pair operators: one contract
PAIR_OPS = ["giou_xyxy", "smooth_l1[0.11]", "smooth_l1[0]", "rotated_iou", "rotated_giou", "rotated_kld"]
PAIR_SIZES = [0, 1, 255, 257, 256 * 1024 + 1]      # the last: the smallest P at which a lane takes a second trip round the grid-stride loop


def _pair_inputs(op, P):
    """Seeded (a, b) on the CPU; rows 0, 1, 2 (where P has them): an identical pair, a disjoint pair, a square box."""
    if op.startswith("smooth_l1"):
        a, b = torch.randn(P, generator=_g(11)), torch.randn(P, generator=_g(12))
        a[:1] = b[:1]
        return a, b
    if op == "giou_xyxy":
        a, b = _boxes(P, 13), _boxes(P, 14)
        a[:1] = b[:1]
        if P > 1:
            a[1] = torch.tensor([0.0, 0.0, 5.0, 5.0]); b[1] = torch.tensor([500.0, 500.0, 560.0, 560.0])
        return a, b
    a = _rboxes(P, 15)
    b = a.clone()
    b[:, :2] += (torch.rand(P, 2, generator=_g(16)) - 0.5) * 20
    b[:, 2:4] *= 0.7 + torch.rand(P, 2, generator=_g(17)) * 0.6
    b[:, 4] += (torch.rand(P, generator=_g(18)) - 0.5) * 40
    b[:1] = a[:1]
    if P > 1:
        b[1, :2] = a[1, :2] + 1000.0
    if P > 2:
        a[2, 3] = a[2, 2]
    return a, b


def _pair_run(op, a, b, grad_scale):
    """-> (elem, sum, gradient w.r.t. a) of one operator through its public op-layer names."""
    from slenderobjdet_amd.layers import functional as HF

    if op == "giou_xyxy":
        return HF.giou_loss_xyxy(a, b, want_grad=True, grad_scale=grad_scale)
    if op.startswith("smooth_l1"):
        return HF.smooth_l1_loss(a, b, float(op[10:-1]), want_grad=True, grad_scale=grad_scale)
    stem = op[len("rotated_"):]
    elem, s = getattr(HF, f"rotated_{stem}_loss_fwd")(a, b)
    return elem, s, getattr(HF, f"rotated_{stem}_loss_bwd")(a, b, grad_scale)


def _pair_sum_roundings(P):
    """Roundings on the longest path from an elem to sum_out, counted in csrc/pair_loss.h and csrc/common.h.  A sum that starts from 0
    rounds once per addend after the first.  Lane loop: T = ceil(P / (256 g)) trips over g = sod_nblk(P) blocks, T - 1 roundings.
    block_sum_256: 6 shuffle steps of wave_sum, then red[0] + red[1] + red[2] + red[3]: 6 + 3 = 9.  sod_finish_sums_kernel: a thread adds
    ceil(g / 256) partials, ceil(g / 256) - 1 roundings, then block_sum_256 again: 9.  (P = 256 * 1024 + 1: 1 + 9 + 3 + 9 = 22.)"""
    g = min(max((P + 255) // 256, 1), 1024)
    trips = (P + 256 * g - 1) // (256 * g)
    return max(trips - 1, 0) + 9 + ((g + 255) // 256 - 1) + 9


@pytest.mark.parametrize("P", PAIR_SIZES)
@pytest.mark.parametrize("op", PAIR_OPS)
def test_pair_operators_one_contract(cuda, op, P):
    """One pair per lane, so no row depends on another: the rows of a call over P pairs that a call over fewer pairs also computes - a
    prefix of 257 and the very last row - carry the same bits there; grad_scale [0.25] scales the gradient exactly; sum_out is the
    float64 sum of elem within the roundings of the reduction; P = 0 gives sum == 0, empty rows and no error."""
    a, b = (t.to(cuda) for t in _pair_inputs(op, P))
    elem, s, d = _pair_run(op, a, b, None)
    assert elem.shape == a.shape[:1] and d.shape == a.shape and s.shape == (1,)
    if P == 0:
        assert s.item() == 0.0
        return
    assert torch.equal(_pair_run(op, a, b, torch.tensor([0.25], device=cuda))[2], d * 0.25)
    for rows in (slice(0, min(P, 257)), slice(P - 1, P)):
        e2, _, d2 = _pair_run(op, a[rows].contiguous(), b[rows].contiguous(), None)
        assert torch.equal(elem[rows], e2) and torch.equal(d[rows], d2), (op, P, rows)
    ref, mag = elem.double().sum().item(), elem.double().abs().sum().item()
    bound = _pair_sum_roundings(P) * 2.0 ** -24 * mag
    print(f"{op} P={P}: |sum - float64 sum| = {abs(s.item() - ref):.3e}, bound {bound:.3e}")
    assert abs(s.item() - ref) <= bound, (op, P, s.item(), ref, bound)


def test_pair_operators_refuse_mismatched_shapes(cuda):
    """The op layer refuses what the kernel would misread: a second tensor with fewer rows (read out of bounds before), and for the XYXY
    GIoU a trailing dimension other than 4."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    b1, b2 = _boxes(9, 1).to(cuda), _boxes(9, 2).to(cuda)
    with pytest.raises(_C.SlenderHipError):
        HF.giou_loss_xyxy(b1, b2[:8].contiguous())
    with pytest.raises(_C.SlenderHipError):
        HF.giou_loss_xyxy(_rboxes(9, 1).to(cuda), _rboxes(9, 2).to(cuda))
    with pytest.raises(_C.SlenderHipError):
        HF.giou_loss_xyxy(b1.view(-1), b2.view(-1))
    x = torch.randn(9, generator=_g(3)).to(cuda)
    with pytest.raises(_C.SlenderHipError):
        HF.smooth_l1_loss(x, x[:8].contiguous(), 0.11)
