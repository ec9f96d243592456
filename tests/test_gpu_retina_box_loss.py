"""The fused RetinaNet box loss (csrc/retina_box_loss.hip): one kernel template, four kinds - smooth-L1 over 4 ("box") and 5 ("box5")
deltas, GIoU ("giou"), rotated IoU ("riou").  What is checked here is the contract the kinds share, on inputs built in the test:
sums[1] = number of positives exactly, the EMA normaliser, sums[0] against a float64 restatement (1e-4 relative, the bar of
test_loss_kernels_vs_restatement), and the backward pass into a buffer of sevens in both storage types: rows of non-positives and pad
columns exactly zero, the same bits from a second call, bf16 = fp32 rounded.  Gradient VALUES against float64 stay with
test_gpu_retinanet.py, test_gpu_rotated_retinanet.py and test_gpu_rotated_iou_loss.py."""
import functools
import math

import pytest
import torch

import rotated_iou_loss_restated as RL

pytestmark = pytest.mark.gpu

KINDS = ("box", "box5", "giou", "riou")
DIM = {"box": 4, "box5": 5, "giou": 4, "riou": 5}
CLAMP = math.log(1000.0 / 16)
BETA, K, MOMENTUM, NORM0 = 0.1, 4, 0.9, 100.0
BWD_SPAN = 4096 * 256           # anchors per trip of the backward grid-stride loop (the forward loop's span is 1024 * 256)


def _shape(kind, case):
    """-> (N, P, A, pitch): "pad" / "nopad" are the small contract case (two levels of 5x7 and 3x4 pixels: N*R = 282, the last
    workgroup is partial), "stride" one 160x160 level whose N*R exceeds both grid-stride spans."""
    D = DIM[kind]
    if case == "stride":
        return (8, 160 * 160, 9, 40) if D == 4 else (8, 160 * 160, 6, 32)
    return 2, 5 * 7 + 3 * 4, 3, (16 if case == "pad" else 3 * D)


@functools.lru_cache(maxsize=None)
def _case(kind, case):
    """Inputs on the device (never written afterwards) and the float64 reference of the forward sum."""
    from oracle import losses as OL
    from oracle import retinanet as orn
    from slenderobjdet_amd.layers import functional as HF

    cuda = torch.device("cuda:0")
    D = DIM[kind]
    N, P, A, pitch = _shape(kind, case)
    R = P * A
    g = torch.Generator().manual_seed(11 + KINDS.index(kind))
    pred = torch.randn(N, P, pitch, generator=g) * 0.2                       # the pad columns hold noise too: nothing may read them
    u = torch.rand(N, R, generator=g)
    if case == "stride":                                                    # ~0.5 % positives, ~1 % ignored
        lab = torch.full((N, R), K, dtype=torch.int32)
        lab[u < 0.015] = -1
        cls = torch.randint(0, K, (N, R), generator=g, dtype=torch.int32)
        lab[u < 0.005] = cls[u < 0.005]
        lab.view(-1)[-3] = 1                                                # a positive in the backward loop's second trip
    else:
        lab = torch.randint(-1, K + 1, (N, R), generator=g, dtype=torch.int32)
    pos = (lab >= 0) & (lab != K)
    assert int(pos.sum()) >= 10 and int((lab == -1).sum()) >= 1 and int((lab == K).sum()) >= 1
    if case == "stride":
        assert N * R > BWD_SPAN and bool(pos.view(-1)[BWD_SPAN:].any())
    pdel = pred[..., : A * D].reshape(N, R, D)
    weights = (1.0,) * D
    if kind in ("box", "box5"):
        anchors, extra = None, (BETA,)
        target = torch.randn(N, R, D, generator=g)
        ref = float(OL.smooth_l1_loss(pdel[pos].double(), target[pos].double(), BETA).sum())
    else:
        uni = lambda lo, hi: lo + (hi - lo) * torch.rand(R, generator=g)
        cx, cy, w, h = uni(16, 240), uni(16, 240), uni(8, 64), uni(8, 64)
        if D == 4:
            anchors = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], 1)
        else:
            anchors = torch.stack([cx, cy, w, h, uni(-90, 90)], 1)
        # the target of every anchor: its own prediction plus small noise, decoded - every positive overlaps its target
        noisy = (pdel + 0.05 * torch.randn(N, R, D, generator=g)).reshape(N * R, D).contiguous()
        arep = anchors.repeat(N, 1)
        target = HF.box2box_apply_deltas(noisy.to(cuda), arep.to(cuda), weights, CLAMP).cpu().view(N, R, D)
        p64, a64, t64 = pdel[pos].double(), arep.view(N, R, D)[pos].double(), target[pos].double()
        if D == 4:
            ref = float(OL.giou_loss_xyxy(orn.apply_deltas(p64, a64, weights, CLAMP), t64).sum())
        else:
            ref = float((1.0 - RL.iou(RL.decode(p64, a64, weights, CLAMP), t64)).sum())
        extra = (anchors.to(cuda), weights, CLAMP)
    return dict(kind=kind, N=N, P=P, A=A, R=R, D=D, pitch=pitch, pred=pred.to(cuda), lab=lab.to(cuda), target=target.contiguous().to(cuda),
                extra=extra, pos=pos, ref=ref)


def _fwd(c, nrm, pred=None, lab=None):
    from slenderobjdet_amd.layers import functional as HF

    pred, lab = c["pred"] if pred is None else pred, c["lab"] if lab is None else lab
    f = getattr(HF, f"retina_{c['kind']}_loss_fwd")
    if len(c["extra"]) == 1:
        return f(pred, c["pitch"], lab, c["target"], c["N"], c["R"], c["A"], K, BETA, nrm, MOMENTUM)
    anchors, weights, clamp = c["extra"]
    return f(pred, c["pitch"], lab, anchors, c["target"], c["N"], c["R"], c["A"], K, weights, clamp, nrm, MOMENTUM)


def _bwd(c, d, pred=None, lab=None):
    from slenderobjdet_amd.layers import functional as HF

    pred, lab = c["pred"] if pred is None else pred, c["lab"] if lab is None else lab
    num, den = torch.ones(1, device=d.device), torch.full((1,), NORM0, device=d.device)
    f = getattr(HF, f"retina_{c['kind']}_loss_bwd")
    if len(c["extra"]) == 1:
        return f(pred, c["pitch"], lab, c["target"], c["N"], c["R"], c["A"], K, BETA, num, den, d)
    anchors, weights, clamp = c["extra"]
    return f(pred, c["pitch"], lab, anchors, c["target"], c["N"], c["R"], c["A"], K, weights, clamp, num, den, d)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check_contract(c, cuda):
    from slenderobjdet_amd.layers import functional as HF

    N, P, A, R, D, pitch, pos = c["N"], c["P"], c["A"], c["R"], c["D"], c["pitch"], c["pos"]
    npos = int(pos.sum())
    nrm = torch.tensor([NORM0], device=cuda)
    sums = _fwd(c, nrm).cpu()
    want_nrm = MOMENTUM * NORM0 + (1.0 - MOMENTUM) * max(npos, 1)
    print(f"\n{c['kind']} N*R {N * R} pitch {pitch}: {npos} positives, sum hip {float(sums[0]):.7f} float64 {c['ref']:.7f}, "
          f"normaliser {float(nrm):.4f} against {want_nrm:.4f}")
    assert float(sums[1]) == npos
    assert abs(float(nrm) - want_nrm) < 1e-3
    assert abs(float(sums[0]) - c["ref"]) <= 1e-4 * max(abs(c["ref"]), 1e-3)
    out = {}
    for mode in ("bf16", "fp32"):
        prev = HF.set_precision(mode)
        try:
            d, d2 = (torch.full((N, P, pitch), 7.0, dtype=HF.ACT_DTYPE, device=cuda) for _ in range(2))
            _bwd(c, d)
            _bwd(c, d2)
        finally:
            HF.set_precision(prev)
        rows = d[..., : A * D].reshape(N, R, D).cpu()
        assert (rows[~pos] == 0).all(), mode                                # every non-positive row: exact zeros over the sevens
        assert (d[..., A * D:] == 0).all(), mode                            # every pad column
        assert torch.equal(_bits(d), _bits(d2)), mode
        out[mode] = d
    assert torch.equal(_bits(out["bf16"]), _bits(out["fp32"].to(torch.bfloat16)))      # the storage type only changes the final cast
    return out["fp32"][..., : A * D].reshape(N * R, D).cpu()


@pytest.mark.parametrize("case", ["pad", "nopad"])
@pytest.mark.parametrize("kind", KINDS)
def test_contract_small(cuda, kind, case):
    """N = 2, 47 pixels, A = 3, K = 4: with pad columns (pitch 16) and without (pitch A*D: the pad loop is empty)."""
    c = _case(kind, case)
    assert c["N"] * c["R"] == 282
    rows = _check_contract(c, cuda)
    assert (rows[c["pos"].view(-1)].abs().sum(1) > 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_contract_both_grid_stride_loops_take_a_second_trip(cuda, kind):
    """One 160x160 level, N = 8: N*R is above the forward span (1024 blocks) and the backward span (4096 blocks); a positive beyond
    anchor 4096 * 256 gets its gradient row."""
    c = _case(kind, "stride")
    rows = _check_contract(c, cuda)
    late = c["pos"].view(-1)[BWD_SPAN:]
    assert bool((rows[BWD_SPAN:][late].abs().sum(1) > 0).any())


@pytest.mark.parametrize("kind", KINDS)
def test_wrappers_refuse_buffers_that_do_not_match_the_integers(cuda, kind):
    """The kernels index by N, R, A and pitch alone: a prediction buffer with one row too few, or labels of another R, is an error on
    the host (no launch) and not an out-of-bounds access."""
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    c = _case(kind, "pad")
    short_pred = c["pred"][:, :-1].contiguous()
    short_lab = c["lab"][:, : -c["A"]].contiguous()
    d = torch.zeros_like(c["pred"], dtype=HF.ACT_DTYPE)
    for kw in (dict(pred=short_pred), dict(lab=short_lab)):
        with pytest.raises(_C.SlenderHipError, match=f"retina_{kind}_loss: pred"):
            _fwd(c, torch.tensor([NORM0], device=cuda), **kw)
        with pytest.raises(_C.SlenderHipError, match=f"retina_{kind}_loss: pred"):
            _bwd(c, d, **kw)
    with pytest.raises(_C.SlenderHipError, match=f"retina_{kind}_loss: pred"):
        _bwd(c, d[:, :-1].contiguous())
