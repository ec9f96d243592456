"""detectron2's DatasetEvaluator / DatasetEvaluators / inference_context and the reference's inference_on_dataset
(slender_det/evaluation/evaluator.py:12-96, argument order (dataset_name, model, data_loader, evaluator))."""
import datetime
import logging
import time
from collections import OrderedDict
from contextlib import contextmanager

import torch

from ..utils.comm import get_world_size, is_main_process


class DatasetEvaluator:
    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        pass


class DatasetEvaluators(DatasetEvaluator):
    def __init__(self, evaluators):
        super().__init__()
        self._evaluators = evaluators

    def reset(self):
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs):
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self):
        results = OrderedDict()
        for e in self._evaluators:
            result = e.evaluate()
            if is_main_process() and result is not None:
                for k, v in result.items():
                    assert k not in results, "Different evaluators produce results with the same key {}".format(k)
                    results[k] = v
        return results


@contextmanager
def inference_context(model):
    training_mode = model.training
    model.eval()
    yield
    model.train(training_mode)


def inference_on_dataset(dataset_name, model, data_loader, evaluator):
    """Run ``model`` in eval mode over ``data_loader`` (an iterable with a length), feed every batch to ``evaluator`` and
    return ``evaluator.evaluate(dataset_name)`` (``evaluate()`` for evaluators that take no name)."""
    num_devices = get_world_size()
    logger = logging.getLogger(__name__)
    total = len(data_loader)
    logger.info("Start inference on {} images".format(total))
    if evaluator is None:
        evaluator = DatasetEvaluators([])
    evaluator.reset()

    num_warmup = min(5, total - 1)
    start_time = time.perf_counter()
    total_compute_time = 0
    with inference_context(model), torch.no_grad():
        for idx, inputs in enumerate(data_loader):
            if idx == num_warmup:
                start_time = time.perf_counter()
                total_compute_time = 0
            outputs = model(inputs)
            start_compute_time = time.perf_counter()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            total_compute_time += time.perf_counter() - start_compute_time
            evaluator.process(inputs, outputs)

    total_time = time.perf_counter() - start_time
    n = max(total - num_warmup, 1)
    logger.info("Total inference time: {} ({:.6f} s / img per device, on {} devices)".format(
        str(datetime.timedelta(seconds=total_time)), total_time / n, num_devices))
    logger.info("Total inference pure compute time: {} ({:.6f} s / img per device, on {} devices)".format(
        str(datetime.timedelta(seconds=int(total_compute_time))), total_compute_time / n, num_devices))
    try:
        results = evaluator.evaluate(dataset_name)
    except TypeError:
        results = evaluator.evaluate()
    if results is None:
        results = {}
    return results
