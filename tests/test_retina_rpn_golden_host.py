"""Pins the CPU oracle of the RetinaNet path and of the RPN / proposal half of the two-stage path (oracle/retinanet.py, oracle/rcnn.py,
oracle/detection.py's matcher and NMS as used there, tests/rotated_retinanet_restated.py) against fixtures produced by the REFERENCE's own
Python (tests/golden/retina_rpn/make_golden_retina_rpn.py; meta.json names the reference lines of every file).  Runs on the CPU.

Integers (labels, matches, kept rows, classes, counts, order) are compared exactly: the generator asserts that none of them hangs on
float rounding.  Floats take the tolerances tests/test_oracle_golden.py holds the head-loss fixtures to: forward values rtol 2e-5 /
atol 1e-6, losses rtol 1e-5, gradients rtol 2e-4 / atol 2e-6 * max(1, |ref|_max).  One value needs more, the angle column of decoded
rotated boxes: its bar is 4x the stored fp32-float64 spread of the reference for that output (boxes_close; measured spread 2.2e-5
degrees).  test_reference_spread_is_below_the_tolerances asserts that every other stored spread lies inside these tolerances, so the
bars are not tighter than the reference's own rounding, and prints the worst ones (forward 0.51, gradients 0.005, losses 0.012 of the bar)."""
import json
import os

import numpy as np
import pytest
import torch

import retinanet_inference_restated as rir
import rotated_retinanet_restated as rrr
from oracle import rcnn as orc
from oracle import retinanet as orn

G = os.path.join(os.path.dirname(__file__), "golden", "retina_rpn")
TAGS = [("xyxy", 4), ("rot", 5)]


def _load(name):
    return {k: v for k, v in np.load(os.path.join(G, name)).items()}


def T(a):
    return torch.from_numpy(np.asarray(a))


def fwd_close(got, ref):
    np.testing.assert_allclose(np.asarray(got), ref, rtol=2e-5, atol=1e-6)


def boxes_close(got, d, key):
    """Decoded boxes.  The angle column of rotated boxes needs more than the head-loss tolerance: it is da * 180 / pi + anchor angle wrapped by
    (a + 180) % 360 - 180, whose fp32 rounding is absolute (an ulp of 360, 3e-5 degrees) however small the angle; the bar there is 4x the
    stored fp32-float64 spread of the reference for that output (measured: 2.2e-5 degrees at most, so the bar is <= 8.7e-5 degrees)."""
    got, ref = np.asarray(got), d[key]
    ok = np.isfinite(ref).all(-1)
    assert (np.isfinite(got).all(-1) == ok).all()
    got, ref, ref64 = got[ok], ref[ok], d[key + "_f64"][ok]
    np.testing.assert_allclose(got[:, :4], ref[:, :4], rtol=2e-5, atol=1e-6)
    if ref.shape[-1] == 5:
        np.testing.assert_allclose(got[:, 4], ref[:, 4], rtol=2e-5, atol=max(1e-6, 4.0 * float(np.abs(ref[:, 4] - ref64[:, 4]).max())))


def loss_close(got, ref):
    np.testing.assert_allclose(float(got), float(ref), rtol=1e-5)


def grad_close(got, ref):
    np.testing.assert_allclose(np.asarray(got), ref, rtol=2e-4, atol=2e-6 * max(1.0, float(np.abs(ref).max())))


def permute_as_the_oracle_does(x, K):
    """oracle/model.py OracleRetinaNet.predictions :345-346: (N, A*K, H, W) -> (N, HWA, K)."""
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, K)


def test_meta_lists_every_fixture_and_every_family():
    meta = json.load(open(os.path.join(G, "meta.json")))
    assert sorted(meta) == sorted(f for f in os.listdir(G) if f.endswith(".npz"))
    for fam in "abcdef":
        lines = [v for v in meta.values() if v.startswith(f"({fam}) reference-Python x restated-op: ")]
        assert lines and all(":" in v.split("restated-op: ")[1].split(" x ")[0] for v in lines), fam      # file:lines


# ------------------------------------------------------------------------------------------------ (a) labels
def test_retina_labels_xyxy():
    d = _load("retina_labels_xyxy.npz")
    anc = T(d["anchors"])
    gtb, gtc = [T(d["gt_boxes0"]), T(d["gt_boxes1"])], [T(d["gt_classes0"]), T(d["gt_classes1"])]
    K = int(d["num_classes"])
    lab, mb = orn.label_anchors(anc, gtb, gtc, list(d["thresholds"]), list(d["iou_labels"]), K)
    np.testing.assert_array_equal(lab.numpy(), d["gt_labels"])
    pos = (lab >= 0) & (lab != K)
    assert pos.sum() > 0 and (lab == -1).sum() > 0 and (lab[1] == K).all()
    np.testing.assert_array_equal(mb[pos].numpy(), d["matched_boxes"][pos.numpy()])       # "undefined" elsewhere (:268)
    np.testing.assert_array_equal(mb[1].numpy(), d["matched_boxes"][1])                    # the empty image: zeros (:289)


def test_retina_labels_rot():
    d = _load("retina_labels_rot.npz")
    anc = T(d["anchors"])
    gtb, gtc = [T(d["gt_boxes0"]), T(d["gt_boxes1"])], [T(d["gt_classes0"]), T(d["gt_classes1"])]
    K = int(d["num_classes"])
    w = (1.0, 1.0, 1.0, 1.0, 1.0)
    lab, deltas, _ = rrr.label_anchors(anc, gtb, gtc, list(d["thresholds"]), list(d["iou_labels"]), K, w)
    np.testing.assert_array_equal(lab.numpy(), d["gt_labels"])
    pos = (lab >= 0) & (lab != K)
    ref = orc.get_deltas(anc, T(d["matched_boxes"][0]), w)
    fwd_close(deltas[0][pos[0]], ref[pos[0]].numpy())
    assert (deltas[1] == 0).all()
    # the same rule through oracle.rcnn's 5-column matcher
    m, ml = orc.rpn_match(anc, gtb[0], tuple(d["thresholds"]), tuple(d["iou_labels"]))
    np.testing.assert_array_equal(gtb[0][m][pos[0]].numpy(), d["matched_boxes"][0][pos[0].numpy()])
    np.testing.assert_array_equal((ml == 1).numpy(), pos[0].numpy())
    np.testing.assert_array_equal((ml == -1).numpy(), d["gt_labels"][0] == -1)


# ------------------------------------------------------------------------------------------------ (b) losses
@pytest.mark.parametrize("kind, tag, D", [("smooth_l1", "xyxy", 4), ("giou", "xyxy", 4), ("smooth_l1", "rot", 5)])
def test_retina_losses(kind, tag, D):
    d = _load(f"retina_losses_{kind}_{tag}.npz")
    K, L = int(d["num_classes"]), len(d["hw"])
    rl = [T(d[f"raw_logits{l}"]).requires_grad_(True) for l in range(L)]
    rd = [T(d[f"raw_deltas{l}"]).requires_grad_(True) for l in range(L)]
    pl, pd = [permute_as_the_oracle_does(x, K) for x in rl], [permute_as_the_oracle_does(x, D) for x in rd]
    for l in range(L):
        np.testing.assert_array_equal(pl[l].detach().numpy(), d[f"logits_perm{l}"])
        np.testing.assert_array_equal(pd[l].detach().numpy(), d[f"deltas_perm{l}"])
    anc, lab, mb = T(d["anchors"]), T(d["gt_labels"]), T(d["matched_boxes"])
    w = tuple(float(v) for v in d["weights"])
    args = (K, float(d["alpha"]), float(d["gamma"]), float(d["beta"]))
    if D == 4:
        out, norm = orn.losses(anc, torch.cat(pl, 1), torch.cat(pd, 1), lab, mb, *args, w, float(d["normalizer_before"]), float(d["momentum"]),
                               box_reg_loss_type=kind)
    else:
        gt_d = torch.stack([orc.get_deltas(anc, m, w) for m in mb])
        gt_d[~((lab >= 0) & (lab != K))] = 0           # rows of non-positives are never read (-inf on the empty image)
        out, norm = rrr.losses(torch.cat(pl, 1), torch.cat(pd, 1), lab, gt_d, *args, float(d["normalizer_before"]), float(d["momentum"]))
    loss_close(out["loss_cls"], d["loss_cls"])
    loss_close(out["loss_box_reg"], d["loss_box_reg"])
    np.testing.assert_allclose(norm, float(d["normalizer_after"]), rtol=1e-6)
    gc = torch.autograd.grad(out["loss_cls"], rl, retain_graph=True)
    gb = torch.autograd.grad(out["loss_box_reg"], rd)
    for l in range(L):
        grad_close(gc[l], d[f"grad_logits{l}"])
        grad_close(gb[l], d[f"grad_deltas{l}"])


# ------------------------------------------------------------------------------------------------ (c) inference
@pytest.mark.parametrize("tag, D", TAGS)
def test_retina_inference(tag, D):
    d = _load(f"retina_inference_{tag}.npz")
    L, K = len(d["hw"]), int(d["num_classes"])
    anc = [T(d[f"anchors{l}"]) for l in range(L)]
    w = tuple(float(v) for v in d["weights"])
    cfg = (float(d["score_threshold"]), int(d["topk_candidates"]), float(d["nms_threshold"]), int(d["max_detections"]))
    for i in range(len(d["image_sizes"])):
        lg, dl = [T(d[f"logits{l}"][i]) for l in range(L)], [T(d[f"deltas{l}"][i]) for l in range(L)]
        if D == 4:
            b, s, c = rir.inference_single_image(anc, lg, dl, K, *cfg, w)
        else:
            keep, B, S, C = rrr.inference_single_image(anc, lg, dl, K, *cfg, w)
            b, s, c = B[keep], S[keep], C[keep]
        np.testing.assert_array_equal(c.numpy(), d[f"classes{i}"])          # same detections in the same order
        fwd_close(s, d[f"scores{i}"])
        boxes_close(b, d, f"boxes{i}")
    if D == 5:
        # the last level alone, more scores above the threshold than top-k, fewer anchors than top-k: the cap by the ANCHOR count (:345) shows
        keep, B, S, C = rrr.inference_single_image(anc[-1:], [T(d["cap_logits"])], [T(d["cap_deltas"])], K, cfg[0], cfg[1], cfg[2],
                                                   int(d["cap_max_detections"]), w)
        assert len(d["cap_scores"]) <= len(anc[-1]) < cfg[1] < int((T(d["cap_logits"]).sigmoid() > cfg[0]).sum())
        np.testing.assert_array_equal(C[keep].numpy(), d["cap_classes"])
        fwd_close(S[keep], d["cap_scores"])
        boxes_close(B[keep], d, "cap_boxes")


# ------------------------------------------------------------------------------------------------ (d) RPN labels and losses
@pytest.mark.parametrize("tag, D", TAGS)
def test_rpn_labels_and_losses(tag, D):
    d = _load(f"rpn_labels_losses_{tag}.npz")
    anc = T(d["anchors"])
    w = tuple(float(v) for v in d["weights"])
    A, L, N = int(d["num_anchors"]), len(d["hw"]), 2
    for i in range(N):
        m, lab = orc.rpn_match(anc, T(d[f"gt_boxes{i}"]), tuple(d["thresholds"]), tuple(d["iou_labels"]))
        np.testing.assert_array_equal(lab.numpy(), d["labels_before_sampling"][i])
        pos = lab == 1
        if len(d[f"gt_boxes{i}"]):
            np.testing.assert_array_equal(T(d[f"gt_boxes{i}"])[m][pos].numpy(), d["matched_boxes"][i][pos.numpy()])
        else:
            assert not d["matched_boxes"][i].any() and (lab == 0).all()
    before, after = d["labels_before_sampling"], d["labels_sampled"]
    # the fill_(-1) / scatter_ contract (:130-133): sampled entries keep their label, the rest is -1
    assert ((after == before) | (after == -1)).all() and ((after >= 0).sum(1) == int(d["batch_size_per_image"])).all()
    rl = [T(d[f"raw_logits{l}"]).requires_grad_(True) for l in range(L)]
    rd = [T(d[f"raw_deltas{l}"]).requires_grad_(True) for l in range(L)]
    # the reshapes as oracle.rcnn.OracleRCNN.rpn_outputs does them (:276-277)
    lg = [x.permute(0, 2, 3, 1).reshape(N, -1) for x in rl]
    dl = [x.view(N, A, D, *x.shape[-2:]).permute(0, 3, 4, 1, 2).reshape(N, -1, D) for x in rd]
    for l in range(L):
        np.testing.assert_array_equal(lg[l].detach().numpy(), d[f"logits_perm{l}"])
        np.testing.assert_array_equal(dl[l].detach().numpy(), d[f"deltas_perm{l}"])
    labels = T(after)
    gt_d = torch.stack([orc.get_deltas(anc, T(mb), w) for mb in d["matched_boxes"]])
    gt_d[labels != 1] = 0
    assert int(d["normalizer"]) == int(d["batch_size_per_image"]) * N
    for name, beta in (("beta0", 0.0), ("beta02", 0.2)):
        out = orc.rpn_losses(torch.cat(lg, 1), torch.cat(dl, 1), labels, gt_d, int(d["batch_size_per_image"]), beta)
        loss_close(out["loss_rpn_cls"], d[f"loss_rpn_cls_{name}"])
        loss_close(out["loss_rpn_loc"], d[f"loss_rpn_loc_{name}"])
        gc = torch.autograd.grad(out["loss_rpn_cls"], rl, retain_graph=True)
        gl = torch.autograd.grad(out["loss_rpn_loc"], rd, retain_graph=True)
        for l in range(L):
            grad_close(gc[l], d[f"grad_logits{l}_{name}"])
            grad_close(gl[l], d[f"grad_deltas{l}_{name}"])


# ------------------------------------------------------------------------------------------------ (e) proposals
@pytest.mark.parametrize("case", ["train", "eval", "nonfinite"])
@pytest.mark.parametrize("tag, D", TAGS)
def test_rpn_proposals(tag, D, case):
    d = _load(f"rpn_proposals_{tag}.npz")
    L = len(d["hw"])
    training, pre, post = json.loads(d["cfg"].item())[case]
    pfx = "nonfinite_" if case == "nonfinite" else ""
    anc = [T(d[f"anchors{l}"]) for l in range(L)]
    lg, dl = [T(d[f"{pfx}logits{l}"]) for l in range(L)], [T(d[f"{pfx}deltas{l}"]) for l in range(L)]
    w = tuple(float(v) for v in d["weights"])
    N = lg[0].shape[0]
    props = [orc.apply_deltas(x.reshape(-1, D), a.repeat(N, 1), w).view(N, -1, D) for x, a in zip(dl, anc)]
    for l in range(L):
        boxes_close(props[l].reshape(-1, D), {k: v.reshape(-1, D) for k, v in d.items() if k.startswith(f"{case}_decoded{l}")}, f"{case}_decoded{l}")
    sizes = [tuple(int(v) for v in s) for s in d["image_sizes"]]
    res = orc.find_top_proposals(props, lg, sizes, float(d["nms_thresh"]), pre, post, float(d["min_box_side_len"]), training)
    all_anc, all_lg = torch.cat(anc), torch.cat(lg, 1)
    for i, (b, s) in enumerate(res):
        assert len(b) == int(d[f"{case}_count{i}"]) == post
        np.testing.assert_array_equal(s.numpy(), d[f"{case}_objectness_logits{i}"])          # same proposals in the same order
        boxes_close(b, d, f"{case}_proposal_boxes{i}")
        assert np.isfinite(b.numpy()).all() and np.isfinite(s.numpy()).all()
        # the reference also returns each proposal's (clipped) anchor: the logits are pairwise distinct, so they name the anchor
        rows = torch.stack([torch.nonzero(all_lg[i] == v)[0, 0] for v in s])
        np.testing.assert_array_equal(orc.clip_boxes(all_anc[rows], sizes[i]).numpy(), d[f"{case}_anchor_boxes{i}"])
    if case == "nonfinite":
        with pytest.raises(FloatingPointError):
            orc.find_top_proposals(props, lg, sizes, float(d["nms_thresh"]), pre, post, float(d["min_box_side_len"]), True)


# ------------------------------------------------------------------------------------------------ (f) Fast R-CNN inference
@pytest.mark.parametrize("name, key, topk", [("specific_top10", "boxes_specific", 10), ("specific_all", "boxes_specific", -1),
                                             ("agnostic_top10", "boxes_agnostic", 10), ("agnostic_all", "boxes_agnostic", -1)])
def test_fast_rcnn_inference(name, key, topk):
    d = _load("fast_rcnn_inference.npz")
    size = tuple(int(v) for v in d["image_size"])
    assert not np.isfinite(d[key]).all()
    b, s, c = orc.fast_rcnn_inference_single_image(T(d[key]), T(d["probs"]), size, float(d["score_thresh"]), float(d["nms_thresh"]), topk, D=4)
    np.testing.assert_array_equal(c.numpy(), d[f"{name}_classes"])
    np.testing.assert_array_equal(s.numpy(), d[f"{name}_scores"])
    fwd_close(b, d[f"{name}_boxes"])
    # rows index the finite inputs (:70-75 filter first); anchors / proposals ride along, clipped
    finite = np.isfinite(d[key]).all(1) & np.isfinite(d["probs"]).all(1)
    rows = d[f"{name}_rows_of_finite_input"]
    np.testing.assert_array_equal(orc.clip_boxes(T(d["proposal_boxes"][finite][rows]), size).numpy(), d[f"{name}_proposals"])
    np.testing.assert_array_equal(orc.clip_boxes(T(d["anchor_boxes"][finite][rows]), size).numpy(), d[f"{name}_anchors"])
    np.testing.assert_array_equal(T(d["probs"][finite][rows, d[f"{name}_classes"]]).numpy(), d[f"{name}_scores"])


# ------------------------------------------------------------------------------------------------ the yardstick
def test_reference_spread_is_below_the_tolerances():
    """|ref32 - ref64| of every stored float output: the reference's own rounding must fit inside the tolerances above."""
    worst = {}
    for f in sorted(os.listdir(G)):
        if not f.endswith(".npz"):
            continue
        d = _load(f)
        for k in d:
            if k + "_f64" not in d:
                continue
            a, b = d[k].astype(np.float64), d[k + "_f64"]
            if a.ndim >= 2 and a.shape[-1] == 5 and ("boxes" in k or "decoded" in k):
                a, b = a[..., :4], b[..., :4]          # the angle column's bar IS 4x this spread (boxes_close)
            ok = np.isfinite(a) & np.isfinite(b)
            assert (np.isfinite(a) == np.isfinite(b)).all(), (f, k)
            if not ok.any():
                continue
            if "grad" in k:
                bar = 2e-4 * np.abs(b[ok]) + 2e-6 * max(1.0, float(np.abs(b[ok]).max()))
            elif "loss" in k or "normalizer" in k:
                bar = 1e-5 * np.abs(b[ok])
            else:
                bar = 2e-5 * np.abs(b[ok]) + 1e-6
            ratio = float((np.abs(a[ok] - b[ok]) / bar).max()) if ok.any() else 0.0
            kind = "grad" if "grad" in k else "loss" if ("loss" in k or "normalizer" in k) else "forward"
            worst[kind] = max(worst.get(kind, (0.0, "")), (ratio, f"{f}:{k}"))
            assert ratio <= 1.0, (f, k, ratio)
    print("\nworst fp32-float64 spread of the reference, as a fraction of the tolerance:", worst)
