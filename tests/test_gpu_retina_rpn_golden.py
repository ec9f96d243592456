"""The product path of RetinaNet / RotatedRetinaNet and of the RPN / proposal half of the two-stage detector against fixtures produced by the
REFERENCE's own Python (tests/golden/retina_rpn/, made by make_golden_retina_rpn.py; tests/test_retina_rpn_golden_host.py holds the CPU
oracle to the same files).  Reads only that folder; builds no backbone: the entry points the models call are run on the fixture's inputs,
methods unbound on a SimpleNamespace ``self`` where they are methods.

Decisions (labels, matches, kept rows, classes, counts, order) are compared exactly: the generator asserts in float64 that none hangs on
rounding.  Value bars are those of the existing test of the same kernel, named at each use."""
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden", "retina_rpn")
SIZES, RATIOS4, RATIOS5, ANGLES = [[16], [32], [64]], [[0.5, 1.0, 2.0]], [[0.5]], [[-45, 0, 45]]      # the generator's anchors


def _load(name):
    return {k: v for k, v in np.load(os.path.join(G, name)).items()}


def T(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dev is not None else t


def _inst(boxes, box_type, dev):
    from slenderobjdet_amd.structures import Instances

    i = Instances((64, 80))
    i.gt_boxes = box_type(T(boxes, dev).float())
    return i


# ------------------------------------------------------------------------------------------------ labels
def test_retina_labels_xyxy(cuda):
    """RetinaNetBase.label_anchors' two kernels (HF.anchor_match + HF.retina_targets)."""
    from oracle import rcnn as orc
    from slenderobjdet_amd.layers import functional as HF

    d = _load("retina_labels_xyxy.npz")
    K, w = int(d["num_classes"]), (1.0, 1.0, 1.0, 1.0)
    anc = T(d["anchors"], cuda)
    R = anc.shape[0]
    for i in range(2):
        boxes, classes = T(d[f"gt_boxes{i}"], cuda).float().contiguous(), T(d[f"gt_classes{i}"], cuda).to(torch.int32).contiguous()
        labels = torch.empty((R,), dtype=torch.int32, device=cuda)
        deltas = torch.empty((R, 4), dtype=torch.float32, device=cuda)
        _, matches, mlab = HF.anchor_match(boxes, anc, [float(v) for v in d["thresholds"]], [int(v) for v in d["iou_labels"]], True)
        HF.retina_targets(anc, boxes, classes, matches, mlab, K, w, labels, deltas)
        ref = d["gt_labels"][i]
        np.testing.assert_array_equal(labels.cpu().numpy(), ref)
        pos = torch.from_numpy((ref >= 0) & (ref != K))
        if pos.any():
            want = orc.get_deltas(T(d["anchors"]), T(d["matched_boxes"][i]), w)[pos]
            # bar: test_gpu_rcnn.py::test_box_coding_matches_oracle (get_deltas rtol 1e-5, atol 1e-5)
            assert torch.allclose(deltas.cpu()[pos], want, rtol=1e-5, atol=1e-5)
            np.testing.assert_array_equal(boxes.cpu()[matches.cpu().long()][pos].numpy(), d["matched_boxes"][i][pos.numpy()])


def test_retina_labels_rot(cuda):
    """RotatedRetinaNet.label_anchors (HF.retina_label_rotated on the padded batch)."""
    from oracle import rcnn as orc
    from slenderobjdet_amd.modeling.meta_arch.rotated_retinanet import RotatedRetinaNet
    from slenderobjdet_amd.structures import Instances, RotatedBoxes

    d = _load("retina_labels_rot.npz")
    K, w = int(d["num_classes"]), (1.0, 1.0, 1.0, 1.0, 1.0)
    inst = []
    for i in range(2):
        g = Instances((64, 80))
        g.gt_boxes, g.gt_classes = RotatedBoxes(T(d[f"gt_boxes{i}"], cuda).float().view(-1, 5)), T(d[f"gt_classes{i}"], cuda)
        inst.append(g)
    self = NS(iou_thresholds=[float(v) for v in d["thresholds"]], iou_labels=[int(v) for v in d["iou_labels"]], num_classes=K,
              bbox_reg_weights=w, box_reg_loss_type="smooth_l1")
    labels, deltas = RotatedRetinaNet.label_anchors(self, T(d["anchors"], cuda), inst)
    np.testing.assert_array_equal(labels.cpu().numpy(), d["gt_labels"])
    pos = torch.from_numpy((d["gt_labels"][0] >= 0) & (d["gt_labels"][0] != K))
    want = orc.get_deltas(T(d["anchors"]), T(d["matched_boxes"][0]), w)[pos]
    # bar: test_gpu_rcnn.py::test_box_coding_matches_oracle (get_deltas rtol 1e-5, atol 1e-5)
    assert pos.any() and torch.allclose(deltas.cpu()[0][pos], want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("tag, D", [("xyxy", 4), ("rot", 5)])
def test_rpn_labels_and_sampled_targets(cuda, tag, D):
    """RPN.label_and_sample_anchors up to the sampler (the device sampler draws its own subset) and RPN.sampled_targets."""
    from oracle import rcnn as orc
    from slenderobjdet_amd.modeling.box_regression import Box2BoxTransform, Box2BoxTransformRotated
    from slenderobjdet_amd.modeling.proposal_generator.rpn import RPN
    from slenderobjdet_amd.structures import Boxes, RotatedBoxes

    d = _load(f"rpn_labels_losses_{tag}.npz")
    w = tuple(float(v) for v in d["weights"])
    S = int(d["batch_size_per_image"])
    anc = T(d["anchors"], cuda)
    inst = [_inst(d[f"gt_boxes{i}"].reshape(-1, D), RotatedBoxes if D == 5 else Boxes, cuda) for i in range(2)]
    self = NS(iou_thresholds=[float(v) for v in d["thresholds"]], iou_labels=[int(v) for v in d["iou_labels"]], batch_size_per_image=S,
              positive_fraction=float(d["positive_fraction"]), box2box_transform=(Box2BoxTransformRotated if D == 5 else Box2BoxTransform)(weights=w))
    labels, matches, idx = RPN.label_and_sample_anchors(self, anc, inst)
    before = d["labels_before_sampling"]
    got = labels.cpu().numpy()
    # rpn.py:130-133: what the sampler keeps has the matcher's label, everything else is -1; the counts are detectron2's
    assert ((got == before) | (got == -1)).all()
    npos = np.minimum((before == 1).sum(1), int(S * float(d["positive_fraction"])))
    np.testing.assert_array_equal((got == 1).sum(1), npos)
    np.testing.assert_array_equal((got == 0).sum(1), np.minimum((before == 0).sum(1), S - npos))
    pos = torch.from_numpy(before[0] == 1)
    np.testing.assert_array_equal(T(d["gt_boxes0"])[matches.cpu()[0].long()][pos].numpy(), d["matched_boxes"][0][pos.numpy()])
    idx, labels_s, deltas_s, _, _ = RPN.sampled_targets(self, anc, inst, labels, matches, idx)
    idx, labels_s, deltas_s = idx.cpu(), labels_s.cpu(), deltas_s.cpu()
    for i in range(2):
        rows = idx[i][idx[i] >= 0].long()
        assert len(rows) == S and (labels_s[i][idx[i] < 0] == -1).all()
        np.testing.assert_array_equal(labels_s[i][: len(rows)].numpy(), got[i][rows.numpy()])
        p = labels_s[i][: len(rows)] == 1
        if p.any():
            want = orc.get_deltas(T(d["anchors"])[rows[p]], T(d["matched_boxes"][i])[rows[p]], w)
            # bar: test_gpu_rcnn.py::test_box_coding_matches_oracle (get_deltas rtol 1e-5, atol 1e-5)
            assert torch.allclose(deltas_s[i][: len(rows)][p], want, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ RetinaNet losses
def _nhwc_pitched(raw_l, pitch):
    """Per-level raw head outputs (N, C, H, W) -> the product's concatenated (N, P, pitch) fp32 buffer (NHWC rows, zero pad)."""
    rows = [x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]) for x in raw_l]
    buf = torch.cat(rows, 1)
    return torch.nn.functional.pad(buf, (0, pitch - buf.shape[-1])).contiguous()


@pytest.mark.parametrize("kind, tag, D", [("smooth_l1", "xyxy", 4), ("giou", "xyxy", 4), ("smooth_l1", "rot", 5)])
def test_retina_loss_kernels(cuda, kind, tag, D):
    """The focal and box-loss forward / backward _RetinaLossFn calls, on the head's raw layout read NHWC and pitched: the row order
    of permute_to_N_HWA_K is the kernels' own indexing."""
    from oracle import rcnn as orc
    from slenderobjdet_amd.layers import functional as HF

    d = _load(f"retina_losses_{kind}_{tag}.npz")
    K, A, L = int(d["num_classes"]), int(d["num_anchors"]), len(d["hw"])
    N = d["raw_logits0"].shape[0]
    w = tuple(float(v) for v in d["weights"])
    cls_buf = _nhwc_pitched([T(d[f"raw_logits{l}"]) for l in range(L)], A * K).to(cuda)
    pitch = (A * D + 7) // 8 * 8
    box_buf = _nhwc_pitched([T(d[f"raw_deltas{l}"]) for l in range(L)], pitch).to(cuda)
    P = cls_buf.shape[1]
    R = P * A
    lab = T(d["gt_labels"]).to(torch.int32).to(cuda).contiguous()
    anc, mb = T(d["anchors"]), T(d["matched_boxes"])
    pos = (T(d["gt_labels"]) >= 0) & (T(d["gt_labels"]) != K)
    if kind == "giou":
        extra, stem, target = (anc.to(cuda), w, orc.SCALE_CLAMP), "giou", mb.to(cuda).contiguous()
    else:
        # the targets the labeller would hand over, rounded to fp32 once (get_deltas evaluated in float64)
        gt_d = torch.stack([orc.get_deltas(anc.double(), m.double(), w) for m in mb]).float()
        gt_d[~pos] = 0
        extra, stem, target = (float(d["beta"]),), ("box5" if D == 5 else "box"), gt_d.to(cuda).contiguous()
    norm = torch.tensor([float(d["normalizer_before"])], device=cuda)
    sums = HF._retina_loss_fwd(stem, D, extra, box_buf, pitch, lab, target, N, R, A, K, norm, float(d["momentum"]))
    focal_sum, _ = HF.focal_loss_fwd(cls_buf.view(N * R, K), lab.view(-1), None, float(d["alpha"]), float(d["gamma"]))
    # bars: test_gpu_retinanet.py::test_retinanet_labels_losses_and_step (losses 1e-4 relative, normaliser 1e-3)
    assert abs(float(norm) - float(d["normalizer_after"])) < 1e-3
    for got, key in ((float(focal_sum[0] / norm), "loss_cls"), (float(sums[0] / norm), "loss_box_reg")):
        ref = float(d[key])
        print(f"\n{kind} {tag} {key}: hip {got:.7f} reference {ref:.7f}")
        assert abs(got - ref) <= 1e-4 * max(abs(ref), 1e-3), (key, got, ref)
    # focal backward as _RetinaLossFn.backward calls it when the one-pass kernel does not apply (K % 4 != 0 here): g / normaliser on the device.
    # bars: test_gpu_losses.py::test_focal_labels (fp32 rows 1e-5, bf16 rows 2^-7, of the largest |reference|); that test has no label -1,
    # so the rows of ignored anchors are held to exactly zero here (retina_rotated.py:208-222: valid_mask feeds the focal loss)
    ref_c = torch.cat([T(d[f"grad_logits{l}"]).permute(0, 2, 3, 1).reshape(N, -1, K) for l in range(L)], 1).reshape(N * R, K)
    ignored = (T(d["gt_labels"]) == -1).reshape(-1)
    assert ignored.any() and (ref_c[ignored] == 0).all() and float(ref_c.abs().max()) > 0
    one = torch.ones(1, device=cuda)
    for bf16, tol in ((False, 1e-5), (True, 2.0 ** -7)):
        gc = HF.focal_loss_bwd(cls_buf.view(N * R, K), lab.view(-1), None, float(d["alpha"]), float(d["gamma"]), scale_num=one, scale_den=norm,
                               den_mul=1.0, den_min=1e-12, out_bf16=bf16).float().cpu()
        err, lim = float((gc - ref_c).abs().max()), tol * float(ref_c.abs().max())
        print(f"{kind} {tag} focal gradient ({'bf16' if bf16 else 'fp32'} rows): max error {err:.3g}, bar {lim:.3g}")
        assert err <= lim, (bf16, err, lim)
        assert (gc[ignored] == 0).all()
    # box-loss backward against float64 autograd through the reference
    ref = torch.cat([T(d[f"grad_deltas{l}_f64"]).permute(0, 2, 3, 1).reshape(N, -1, D) for l in range(L)], 1)
    assert (ref[~pos] == 0).all()
    if kind == "giou":
        dbox = torch.zeros((N, P, pitch), dtype=HF.ACT_DTYPE, device=cuda)
        HF._retina_loss_bwd(stem, D, extra, box_buf, pitch, lab, target, N, R, A, K, one, norm, dbox)
        got = dbox.double().cpu()[..., : A * D].reshape(N, R, D)
        # bar: test_gpu_retinanet.py::test_retinanet_giou_regression_vs_oracle (bf16 gradient rows: rtol 2e-2, atol 2e-5; zero off the positives)
        assert torch.allclose(got[pos], ref[pos], rtol=2e-2, atol=2e-5) and (got[~pos] == 0).all() and (dbox[..., A * D:] == 0).all()
        return
    # bars: test_gpu_rotated_retinanet.py::test_loss_kernels_vs_restatement (rows of the positives relative to their norm: 4e-3 with bf16
    # storage, 2e-6 with fp32 storage; every other row and the pad columns exactly zero)
    for mode, tol in (("bf16", 4e-3), ("fp32", 2e-6)):
        prev = HF.set_precision(mode)
        try:
            dbox = torch.zeros((N, P, pitch), dtype=HF.ACT_DTYPE, device=cuda)
            HF._retina_loss_bwd(stem, D, extra, box_buf, pitch, lab, target, N, R, A, K, one, norm, dbox)
        finally:
            HF.set_precision(prev)
        got = dbox.double().cpu()[..., : A * D].reshape(N, R, D)
        rel = float((got - ref)[pos].norm() / ref[pos].norm())
        print(f"{kind} {tag} {mode}: delta-gradient rows of {int(pos.sum())} positives off by {rel:.3g} of their norm")
        assert rel <= tol, (mode, rel)
        assert (got[~pos] == 0).all() and (dbox[..., A * D:] == 0).all()


# ------------------------------------------------------------------------------------------------ RPN losses
@pytest.mark.parametrize("tag, D", [("xyxy", 4), ("rot", 5)])
def test_rpn_loss_kernels(cuda, tag, D):
    """bce_logits_loss_* / rpn_loc_loss_* on the rows of the fixture's sampled anchors, taken from the raw head layout by
    rpn_gather_sampled (positives first, index order: the list sod_sample_labels_list writes)."""
    from oracle import rcnn as orc
    from slenderobjdet_amd.layers import functional as HF

    d = _load(f"rpn_labels_losses_{tag}.npz")
    A, L, S = int(d["num_anchors"]), len(d["hw"]), int(d["batch_size_per_image"])
    N = d["raw_logits0"].shape[0]
    w = tuple(float(v) for v in d["weights"])
    labels = T(d["labels_sampled"])
    idx = torch.stack([torch.cat((torch.nonzero(l == 1)[:, 0], torch.nonzero(l == 0)[:, 0])) for l in labels]).to(torch.int32)
    assert idx.shape == (N, S)
    pad = lambda x, c: torch.nn.functional.pad(x.permute(0, 2, 3, 1), (0, c - x.shape[1])).contiguous()
    logits_l = [pad(T(d[f"raw_logits{l}"]), (A + 7) // 8 * 8).to(cuda) for l in range(L)]
    deltas_l = [pad(T(d[f"raw_deltas{l}"]), (A * D + 7) // 8 * 8).to(cuda) for l in range(L)]
    lg, dl = HF.rpn_gather_sampled(logits_l, deltas_l, idx.to(cuda), A, D)
    ref_lg = torch.gather(torch.cat([T(d[f"logits_perm{l}"]) for l in range(L)], 1), 1, idx.long())
    ref_dl = torch.gather(torch.cat([T(d[f"deltas_perm{l}"]) for l in range(L)], 1), 1, idx.long()[:, :, None].expand(-1, -1, D))
    assert torch.equal(lg.cpu(), ref_lg) and torch.equal(dl.cpu(), ref_dl)          # the reshapes of forward (:278-289) as the gather's row order
    labels_s = torch.gather(labels, 1, idx.long()).contiguous().to(cuda)
    anc = T(d["anchors"])
    tgt = torch.stack([orc.get_deltas(anc[idx[i].long()], T(d["matched_boxes"][i])[idx[i].long()], w) for i in range(N)])
    tgt[labels_s.cpu() != 1] = 0
    tgt = tgt.contiguous().to(cuda)
    norm = float(d["normalizer"])
    one = torch.ones(1, device=cuda)
    gl_ref = lambda name: torch.gather(torch.cat([T(d[f"grad_logits{l}_{name}"]).permute(0, 2, 3, 1).reshape(N, -1) for l in range(L)], 1), 1, idx.long())
    gd_ref = lambda name: torch.gather(torch.cat([T(d[f"grad_deltas{l}_{name}"]).view(N, A, D, *d["hw"][l]).permute(0, 3, 4, 1, 2).reshape(N, -1, D)
                                                  for l in range(L)], 1), 1, idx.long()[:, :, None].expand(-1, -1, D))
    for name, beta in (("beta0", 0.0), ("beta02", 0.2)):
        s_cls, s_loc = HF.bce_logits_loss_fwd(lg, labels_s), HF.rpn_loc_loss_fwd(dl, tgt, labels_s, beta)
        # bars: test_gpu_rcnn.py::test_rcnn_loss_kernels_match_torch (sums 1e-4 relative; gradients rtol 1e-5, atol 1e-6)
        for got, key in ((float(s_cls) / norm, f"loss_rpn_cls_{name}"), (float(s_loc) / norm, f"loss_rpn_loc_{name}")):
            ref = float(d[key])
            print(f"\n{tag} {key}: hip {got:.7f} reference {ref:.7f}")
            assert abs(got - ref) < 1e-4 * ref, (key, got, ref)
        assert torch.allclose(HF.bce_logits_loss_bwd(lg, labels_s, one, 1.0 / norm).cpu(), gl_ref(name), rtol=1e-5, atol=1e-6)
        assert torch.allclose(HF.rpn_loc_loss_bwd(dl, tgt, labels_s, beta, one, 1.0 / norm).cpu(), gd_ref(name), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ RetinaNet inference
@pytest.mark.parametrize("tag, D", [("xyxy", 4), ("rot", 5)])
def test_retina_inference(cuda, tag, D):
    """RetinaNetBase.inference (dense_topk_select, decode, batched_nms_topk) / RotatedRetinaNet.inference (retina_decode_rotated): the same
    detections in the same order."""
    from slenderobjdet_amd.modeling.meta_arch.retinanet import RetinaNetBase
    from slenderobjdet_amd.modeling.meta_arch.rotated_retinanet import RotatedRetinaNet

    d = _load(f"retina_inference_{tag}.npz")
    L, K, A = len(d["hw"]), int(d["num_classes"]), 3
    hw = [tuple(int(v) for v in s) for s in d["hw"]]
    N = d["logits0"].shape[0]
    anchors = torch.cat([T(d[f"anchors{l}"]) for l in range(L)]).to(cuda)
    cls_buf = torch.cat([T(d[f"logits{l}"]).reshape(N, -1, A * K) for l in range(L)], 1).contiguous().to(cuda)
    pitch = (A * D + 7) // 8 * 8
    box_buf = torch.nn.functional.pad(torch.cat([T(d[f"deltas{l}"]).reshape(N, -1, A * D) for l in range(L)], 1), (0, pitch - A * D)).contiguous().to(cuda)
    self = NS(head=NS(num_anchors=A), num_classes=K, bbox_reg_weights=tuple(float(v) for v in d["weights"]), strides=[8, 16, 32], anchor_sizes=SIZES,
              anchor_ratios=RATIOS4, anchor_offset=0.0, device=cuda, score_threshold=float(d["score_threshold"]),
              topk_candidates=int(d["topk_candidates"]), nms_threshold=float(d["nms_threshold"]), max_detections_per_image=int(d["max_detections"]),
              scale_clamp=float(np.log(1000.0 / 16)), anchors_for=lambda level_hw: anchors)
    sizes = [tuple(int(v) for v in s) for s in d["image_sizes"]]
    if D == 4:
        from slenderobjdet_amd.modeling.anchor_generator import grid_anchors

        # the fixture's anchors are the product's (an ulp of the cell sizes' square roots at the most)
        assert torch.allclose(torch.cat(grid_anchors(hw, self.strides, SIZES, RATIOS4, 0.0, cuda)), anchors, rtol=0, atol=1e-5)
        res = RetinaNetBase.inference(self, hw, cls_buf, box_buf, None, sizes)
    else:
        res = RotatedRetinaNet.inference(self, hw, cls_buf, box_buf, None, sizes)
    for i, r in enumerate(res):
        np.testing.assert_array_equal(r.pred_classes.cpu().numpy(), d[f"classes{i}"])
        # bars: scores 1e-5 (test_gpu_rotated_retinanet.py::test_inference_matches_the_restatement); boxes rtol 1e-4 / atol 1e-3, the
        # apply_deltas bar of test_gpu_rcnn.py::test_box_coding_matches_oracle (tighter than the 1e-3 relative of the former test)
        assert float((r.scores.cpu() - T(d[f"scores{i}"])).abs().max()) <= 1e-5
        assert torch.allclose(r.pred_boxes.tensor.cpu(), T(d[f"boxes{i}"]), rtol=1e-4, atol=1e-3)


def test_retina_inference_rot_level_with_fewer_anchors_than_topk(cuda):
    """The fixture's one-level case: 18 anchors, 90 scores of which more than top-k pass the threshold; the level's top-k is capped by its
    anchors (retina_rotated.py:345), so at most 18 detections come out."""
    from slenderobjdet_amd.modeling.meta_arch.rotated_retinanet import RotatedRetinaNet

    d = _load("retina_inference_rot.npz")
    K, A, D = int(d["num_classes"]), 3, 5
    L = len(d["hw"])
    hw = [tuple(int(v) for v in d["hw"][-1])]
    anchors = T(d[f"anchors{L - 1}"], cuda)
    cls_buf = T(d["cap_logits"]).reshape(1, -1, A * K).contiguous().to(cuda)
    box_buf = torch.nn.functional.pad(T(d["cap_deltas"]).reshape(1, -1, A * D), (0, 1)).contiguous().to(cuda)
    self = NS(head=NS(num_anchors=A), num_classes=K, bbox_reg_weights=tuple(float(v) for v in d["weights"]), score_threshold=float(d["score_threshold"]),
              topk_candidates=int(d["topk_candidates"]), nms_threshold=float(d["nms_threshold"]), max_detections_per_image=int(d["cap_max_detections"]),
              scale_clamp=float(np.log(1000.0 / 16)), anchors_for=lambda level_hw: anchors)
    (r,) = RotatedRetinaNet.inference(self, hw, cls_buf, box_buf, None, [(64, 80)])
    assert len(r) == len(d["cap_scores"]) <= anchors.shape[0]
    np.testing.assert_array_equal(r.pred_classes.cpu().numpy(), d["cap_classes"])
    # bars: as in test_retina_inference
    assert float((r.scores.cpu() - T(d["cap_scores"])).abs().max()) <= 1e-5
    assert torch.allclose(r.pred_boxes.tensor.cpu(), T(d["cap_boxes"]), rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------ proposals, Fast R-CNN inference
@pytest.mark.parametrize("case", ["train", "eval", "nonfinite"])
@pytest.mark.parametrize("tag, D", [("xyxy", 4), ("rot", 5)])
def test_rpn_proposals(cuda, tag, D, case):
    """RPN.predict_proposals / RRPN on the fixture's logits and deltas: the same boxes and logits in the same order, non-finite rows dropped."""
    from slenderobjdet_amd.modeling.box_regression import Box2BoxTransform, Box2BoxTransformRotated
    from slenderobjdet_amd.modeling.proposal_generator.rpn import RPN
    from slenderobjdet_amd.structures import Boxes, RotatedBoxes

    d = _load(f"rpn_proposals_{tag}.npz")
    L, A = len(d["hw"]), int(d["num_anchors"])
    training, pre, post = json.loads(d["cfg"].item())[case]
    pfx = "nonfinite_" if case == "nonfinite" else ""
    N = d["logits0"].shape[0]
    anchors_l = [T(d[f"anchors{l}"], cuda) for l in range(L)]
    logits_l = [T(d[f"{pfx}logits{l}"]).reshape(N, *d["hw"][l], A).contiguous().to(cuda) for l in range(L)]
    deltas_l = [T(d[f"{pfx}deltas{l}"]).reshape(N, *d["hw"][l], A * D).contiguous().to(cuda) for l in range(L)]
    w = tuple(float(v) for v in d["weights"])
    self = NS(head=NS(num_anchors=A, box_dim=D), training=training, box2box_transform=(Box2BoxTransformRotated if D == 5 else Box2BoxTransform)(weights=w),
              pre_nms_topk={training: pre}, post_nms_topk={training: post}, nms_thresh=float(d["nms_thresh"]), min_box_size=float(d["min_box_side_len"]),
              _box_type=lambda: RotatedBoxes if D == 5 else Boxes)
    res = RPN.predict_proposals(self, anchors_l, logits_l, deltas_l, [tuple(int(v) for v in s) for s in d["image_sizes"]])
    for i, r in enumerate(res):
        assert len(r) == int(d[f"{case}_count{i}"])
        np.testing.assert_array_equal(r.objectness_logits.cpu().numpy(), d[f"{case}_objectness_logits{i}"])
        # bar: test_gpu_rcnn.py::test_box_coding_matches_oracle (apply_deltas rtol 1e-4, atol 1e-3)
        assert torch.allclose(r.proposal_boxes.tensor.cpu(), T(d[f"{case}_proposal_boxes{i}"]), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("name, key, topk", [("specific_top10", "boxes_specific", 10), ("specific_all", "boxes_specific", -1),
                                             ("agnostic_top10", "boxes_agnostic", 10), ("agnostic_all", "boxes_agnostic", -1)])
def test_fast_rcnn_inference(cuda, name, key, topk):
    from slenderobjdet_amd.modeling.roi_heads import fast_rcnn_inference_single_image

    d = _load("fast_rcnn_inference.npz")
    r = fast_rcnn_inference_single_image(T(d[key], cuda), T(d["probs"], cuda), tuple(int(v) for v in d["image_size"]), float(d["score_thresh"]),
                                         float(d["nms_thresh"]), topk)
    np.testing.assert_array_equal(r.pred_classes.cpu().numpy(), d[f"{name}_classes"])
    np.testing.assert_array_equal(r.scores.cpu().numpy(), d[f"{name}_scores"])          # copies of the inputs
    np.testing.assert_array_equal(r.pred_boxes.tensor.cpu().numpy(), d[f"{name}_boxes"])          # clipped copies of the inputs
