from .rotated_coco import coco_to_rotated
from .samplers import RepeatFactorTrainingSampler, TrainingSampler, repeat_factors_from_ratios
from .synthetic import SyntheticCocoBatches, synthetic_batch
from .transforms import DeviceInputPipeline, pil_bilinear_coeffs, resize_shortest_edge_size, transform_boxes
