"""Slender-object COCO box evaluation (slender_det/evaluation): COCOEvaluator with ratio-bucketed AP / AR and the ratio x area
bucketed recall pass, run by three HIP kernels (csrc/coco_eval.hip); RotatedCOCOEvaluator for (cx, cy, w, h, angle) boxes
(csrc/coco_eval_rotated.hip); the evaluator plumbing of detectron2 / the reference."""
from .coco_evaluation import COCOEvaluator
from .evaluator import DatasetEvaluator, DatasetEvaluators, inference_context, inference_on_dataset
from .rotated_coco_evaluation import RotatedCOCOEvaluator

__all__ = ["COCOEvaluator", "DatasetEvaluator", "DatasetEvaluators", "RotatedCOCOEvaluator", "inference_context",
           "inference_on_dataset"]
