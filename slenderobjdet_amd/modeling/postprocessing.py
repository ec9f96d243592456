"""detectron2.modeling.postprocessing.detector_postprocess (call site fcosv2.py:262): rescale boxes to the requested
output resolution, clip, drop empty ones."""
import torch

from ..layers import functional as HF
from ..structures import Boxes, Instances


def detector_postprocess(results, output_height, output_width):
    scale_x = output_width / results.image_size[1]
    scale_y = output_height / results.image_size[0]
    results = Instances((output_height, output_width), **results.get_fields())
    boxes = results.pred_boxes if results.has("pred_boxes") else results.proposal_boxes
    boxes.scale(scale_x, scale_y)
    boxes.clip(results.image_size)
    return results[boxes.nonempty()]


def batched_nms_instances(boxes, scores, classes, iou_threshold, max_keep, image_sizes, extra=None):
    """Class-aware NMS + top-``max_keep`` of padded per-image candidates (boxes (N, M, 4), scores (N, M) with -inf = empty slot,
    classes (N, M) int32) -> one Instances per image with pred_boxes, scores, pred_classes and every (N, M, 4) tensor of ``extra``
    under its key.  Everything stays on the device; the only host read is the per-image detection counts."""
    keep, nkeep = HF.batched_nms_topk(boxes, scores, classes, iou_threshold, max_keep)
    keep4 = keep[:, :, None].expand(-1, -1, 4)
    kb, ks, kc = torch.gather(boxes, 1, keep4), torch.gather(scores, 1, keep), torch.gather(classes, 1, keep)
    kx = {name: torch.gather(t, 1, keep4) for name, t in (extra or {}).items()}
    nk = nkeep.cpu().tolist()
    results = []
    for i, image_size in enumerate(image_sizes):
        r = Instances(tuple(image_size))
        r.pred_boxes, r.scores, r.pred_classes = Boxes(kb[i, : nk[i]]), ks[i, : nk[i]], kc[i, : nk[i]].long()
        for name, t in kx.items():
            r.set(name, t[i, : nk[i]])
        results.append(r)
    return results
