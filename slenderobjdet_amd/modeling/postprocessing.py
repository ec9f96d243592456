"""detectron2.modeling.postprocessing.detector_postprocess (call site fcosv2.py:262): rescale boxes to the requested
output resolution, clip, drop empty ones."""
import torch

from ..layers import functional as HF
from ..structures import Boxes, Instances, RotatedBoxes


def detector_postprocess(results, output_height, output_width):
    scale_x = output_width / results.image_size[1]
    scale_y = output_height / results.image_size[0]
    results = Instances((output_height, output_width), **results.get_fields())
    boxes = results.pred_boxes if results.has("pred_boxes") else results.proposal_boxes
    boxes.scale(scale_x, scale_y)
    boxes.clip(results.image_size)
    return results[boxes.nonempty()]


def batched_nms_instances(boxes, scores, classes, iou_threshold, max_keep, image_sizes, extra=None, box_dim=4):
    """Class-aware NMS + top-``max_keep`` of padded per-image candidates (boxes (N, M, 4), scores (N, M) with -inf = empty slot,
    classes (N, M) int32) -> one Instances per image with pred_boxes, scores, pred_classes and every (N, M, 4) tensor of ``extra``
    under its key.  Everything stays on the device; the only host read is the per-image detection counts.  ``box_dim=5``: boxes
    (N, M, 5) are (cx, cy, w, h, angle_deg), the NMS is the rotated one and pred_boxes are RotatedBoxes (RotatedRetinaNet)."""
    if box_dim not in (4, 5) or boxes.shape[-1] != box_dim:
        raise ValueError(f"batched_nms_instances: boxes {tuple(boxes.shape)} do not have box_dim={box_dim} columns")
    keep, nkeep = HF.batched_nms_topk(boxes, scores, classes, iou_threshold, max_keep)
    keep4 = keep[:, :, None].expand(-1, -1, 4)
    keepb = keep4 if box_dim == 4 else keep[:, :, None].expand(-1, -1, 5)
    wrap = Boxes if box_dim == 4 else RotatedBoxes
    kb, ks, kc = torch.gather(boxes, 1, keepb), torch.gather(scores, 1, keep), torch.gather(classes, 1, keep)
    kx = {name: torch.gather(t, 1, keep4) for name, t in (extra or {}).items()}
    nk = nkeep.cpu().tolist()
    results = []
    for i, image_size in enumerate(image_sizes):
        r = Instances(tuple(image_size))
        r.pred_boxes, r.scores, r.pred_classes = wrap(kb[i, : nk[i]]), ks[i, : nk[i]], kc[i, : nk[i]].long()
        for name, t in kx.items():
            r.set(name, t[i, : nk[i]])
        results.append(r)
    return results
