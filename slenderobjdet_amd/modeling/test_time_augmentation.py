"""Test-time augmentation: ``detectron2.modeling.GeneralizedRCNNWithTTA`` / ``DatasetMapperTTA`` as the reference's
``Trainer.test_with_TTA`` uses them (train_net.py:128-141): every image is run at ``cfg.TEST.AUG.MIN_SIZES`` shortest-edge sizes, each
with and without a horizontal flip, and the detections of all runs are merged by ONE class-aware NMS at the image's output size.
detectron2's source is absent; the semantics are restated in DESIGN.md section 12.

Everything between the decoded uint8 image and the final ``Instances`` stays on the device: ``DeviceInputPipeline`` resizes / flips /
normalises / pads ``batch_size`` copies per launch, the model takes them as ``structures.PreparedInputs``, ``HF.tta_merge_candidates``
(csrc/tta.hip) un-flips, rescales, clips and packs the detections of all runs in one launch, ``batched_nms_instances`` finishes.

One mapping stands for detectron2's ``pre_tfm + resize + flip`` inverse: detectron2 maps augmented -> dataset-mapper input -> output
size with two float32 multiplies; here the augmented box goes to (height, width) with one multiply by ``width / w_a`` (``height /
h_a``), rounded once from double.  The two agree within one float32 rounding of a coordinate.
"""
import torch
from torch import nn

from ..data.transforms import DeviceInputPipeline, resize_shortest_edge_size
from ..layers import functional as HF
from ..structures import ImageList, PreparedInputs
from .postprocessing import batched_nms_instances

SCORE_THRESH = 1e-8     # detectron2 _merge_detections -> fast_rcnn_inference_single_image(..., score_thresh=1e-8, ...)


def tta_plan(h, w, min_sizes, max_size, flip):
    """The augmentations of an (h, w) image in DatasetMapperTTA's order: for every min size the resized run, then (``flip``) the
    resized + mirrored one.  -> [(newh, neww, flip)] with the sizes of ResizeShortestEdge(min_size, max_size)."""
    plan = []
    for size in min_sizes:
        newh, neww = resize_shortest_edge_size(int(h), int(w), int(size), int(max_size))
        plan.append((newh, neww, False))
        if flip:
            plan.append((newh, neww, True))
    return plan


class DatasetMapperTTA:
    """detectron2.modeling.DatasetMapperTTA: holds ``cfg.TEST.AUG``; called with a dataset dict whose "image" is a (3, H, W) tensor it
    returns the plan of that image (``tta_plan``) - the pixels are produced on the device by the wrapper, not here."""

    def __init__(self, cfg):
        aug = cfg.TEST.AUG
        self.min_sizes, self.max_size, self.flip = tuple(aug.MIN_SIZES), int(aug.MAX_SIZE), bool(aug.FLIP)

    def __call__(self, dataset_dict):
        image = dataset_dict["image"]
        return tta_plan(int(image.shape[-2]), int(image.shape[-1]), self.min_sizes, self.max_size, self.flip)


def _nms_thresh_of(cfg, model):
    """The threshold of the merging NMS, or a ValueError that says why this model is refused."""
    from .meta_arch.fcos import FCOSV2
    from .meta_arch.rcnn import GeneralizedRCNN, ProposalNetwork
    from .meta_arch.reppoints import RepPointsDetector
    from .meta_arch.retinanet import RetinaNet

    name = type(model).__name__
    if isinstance(model, ProposalNetwork):
        raise ValueError("GeneralizedRCNNWithTTA: ProposalNetwork yields proposals, not detections - there is nothing to merge")
    if isinstance(model, GeneralizedRCNN):
        if getattr(model.roi_heads, "rotated", False) or getattr(getattr(model.roi_heads, "box_predictor", None), "box_dim", 4) == 5:
            raise ValueError("GeneralizedRCNNWithTTA: rotated boxes (RROIHeads, five-column boxes) are not supported - the merge step "
                             "un-flips and rescales XYXY boxes only")
        return float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
    if isinstance(model, FCOSV2):                       # FCOSV2, FCOS, FCOSTopK, FCOSRepPoints
        return float(model.nms_thresh)
    if isinstance(model, (RetinaNet, RepPointsDetector)):
        return float(model.nms_threshold)
    raise ValueError(f"GeneralizedRCNNWithTTA: {name} is not supported (GeneralizedRCNN, ProposalVisibleRCNN, the FCOS family, RetinaNet "
                     "and RepPointsDetector are)")


class GeneralizedRCNNWithTTA(nn.Module):
    """``GeneralizedRCNNWithTTA(cfg, model)(batched_inputs) -> [{"instances": Instances}]`` with the boxes at each input's
    ("height", "width") (default: the image's own shape).  Beyond detectron2, which asserts a GeneralizedRCNN, the dense detectors are
    accepted (they are merged at their own NMS threshold); rotated configurations, ProposalNetwork and any other class are refused at
    construction.  "image" must be a (3, H, W) uint8 tensor; box detections only (no mask / keypoint pass)."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3):
        super().__init__()
        if isinstance(model, nn.parallel.DistributedDataParallel):
            model = model.module
        self.nms_thresh = _nms_thresh_of(cfg, model)
        self.cfg = cfg.clone() if hasattr(cfg, "clone") else cfg
        self.model = model
        self.tta_mapper = DatasetMapperTTA(cfg) if tta_mapper is None else tta_mapper
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= 64:
            raise ValueError("GeneralizedRCNNWithTTA: batch_size must be in 1..64")
        self.max_detections = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        self.pipeline = DeviceInputPipeline(pixel_mean=model._mean, pixel_std=model._std, size_divisibility=model.backbone.size_divisibility)

    def __call__(self, batched_inputs):
        return [self._inference_one_image(x) for x in batched_inputs]

    @torch.no_grad()
    def _run_model(self, hwc, plan):
        """-> per run (boxes (n, 4), scores (n), classes (n)) in the augmented image's pixels."""
        was_training = self.model.training
        self.model.eval()
        out = []
        try:
            for i in range(0, len(plan), self.batch_size):
                group = plan[i:i + self.batch_size]
                batch, sizes, _, _ = self.pipeline([hwc] * len(group), choices=group)
                if batch.dtype != HF.ACT_DTYPE:      # fp32 validation mode: the pipeline's kernel writes bf16
                    batch = batch.to(HF.ACT_DTYPE)
                # height / width = the augmented size: the model's own postprocess is then an identity scale
                prepared = PreparedInputs([{"height": h, "width": w} for h, w in sizes], ImageList(batch, sizes))
                for res in self.model(prepared):
                    r = res["instances"]
                    out.append((r.pred_boxes.tensor, r.scores, r.pred_classes))
        finally:
            self.model.train(was_training)
        return out

    @torch.no_grad()
    def _inference_one_image(self, inp):
        image = inp.get("image")
        if image is None:
            raise ValueError('GeneralizedRCNNWithTTA: every input needs "image" (reading "file_name" from disk is not supported)')
        if not (torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[0] == 3):
            raise ValueError('GeneralizedRCNNWithTTA: "image" must be a (3, H, W) uint8 tensor')
        height, width = int(inp.get("height", image.shape[1])), int(inp.get("width", image.shape[2]))
        plan = [(int(h), int(w), bool(f)) for h, w, f in self.tta_mapper(inp)]
        if not 1 <= len(plan) <= HF.TTA_MAX_RUNS:
            raise ValueError(f"GeneralizedRCNNWithTTA: 1..{HF.TTA_MAX_RUNS} augmentations per image, got {len(plan)}")
        hwc = image.to(self.model.device, non_blocking=True).permute(1, 2, 0).contiguous()
        dets = self._run_model(hwc, plan)
        counts = [int(d[1].shape[0]) for d in dets]
        det_off = [0]
        for c in counts:
            det_off.append(det_off[-1] + c)
        boxes = torch.cat([d[0].reshape(-1, 4).float() for d in dets]).contiguous()
        scores = torch.cat([d[1].float() for d in dets]).contiguous()
        classes = torch.cat([d[2].to(torch.int32) for d in dets]).contiguous()
        runs = [(0, a, h, w, f) for a, (h, w, f) in enumerate(plan)]
        cand = HF.tta_merge_candidates(boxes, scores, classes, det_off, runs, [(height, width)], len(plan), max(max(counts), 1), SCORE_THRESH)
        return {"instances": batched_nms_instances(*cand, self.nms_thresh, self.max_detections, [(height, width)])[0]}
