"""RetinaNet.inference_single_image (retina_rotated.py:319-378) for axis-aligned boxes restated on the CPU from pieces the tests already trust
(oracle.rcnn.apply_deltas, oracle.detection.batched_nms): the decode / top-k / NMS contract tests/test_gpu_retinanet.py holds the product to
and tests/test_retina_rpn_golden_host.py holds to the reference's own output (tests/golden/retina_rpn/retina_inference_xyxy.npz).
The five-column twin is tests/rotated_retinanet_restated.py."""
import torch

from oracle import detection as od
from oracle import rcnn as orc


def inference_single_image(level_anchors, level_logits, level_deltas, num_classes, score_thresh, topk, nms_thresh, max_det, weights):
    """Per level: sigmoid over (HWA x K), the best min(topk, number of ANCHORS of the level) scores, score threshold, decode; then class-aware
    NMS and the best max_det.  level_logits (HWA, K) or flat, level_deltas (HWA, 4) -> (boxes, scores, classes) in output order."""
    B, S, C = [], [], []
    for anc, logit, delta in zip(level_anchors, level_logits, level_deltas):
        delta = delta.reshape(-1, 4)
        p = logit.reshape(-1).sigmoid()
        k = min(topk, delta.shape[0])
        prob, idx = p.sort(descending=True)
        prob, idx = prob[:k], idx[:k]
        keep = prob > score_thresh
        prob, idx = prob[keep], idx[keep]
        B.append(orc.apply_deltas(delta[idx // num_classes], anc[idx // num_classes], weights))
        S.append(prob)
        C.append(idx % num_classes)
    B, S, C = torch.cat(B), torch.cat(S), torch.cat(C)
    keep = od.batched_nms(B, S, C, nms_thresh)[:max_det]
    return B[keep], S[keep], C[keep]
