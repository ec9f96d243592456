"""Index samplers of the reference's training loader (slender_det/data/build.py): detectron2's TrainingSampler and
RepeatFactorTrainingSampler, and the repeat factors of the reference's "RatioFactorTrainingSampler", which shows images with slender
objects more often.  They yield dataset indices; there is no image loader here."""
import itertools
import os

import torch


def _resolve_seed(seed, world_size):
    """detectron2 draws one seed and shares it among the ranks; here several ranks must be given the seed they share."""
    if seed is not None:
        return int(seed)
    if world_size > 1:
        raise ValueError("the ranks of one job must share a seed: pass seed=")
    return int.from_bytes(os.urandom(4), "little")


def repeat_factors_from_ratios(dataset_dicts_or_json, device=None):
    """float32 [images]: 1 for an image with an annotation of oriented ratio < 1/5, else 0.5 with one < 1/3, else 0.1
    (build.py:16-28).  The input is a list of dataset dicts with ``annotations``, or a COCO json (a path or a dict), whose images
    count in the order of its ``images`` list.  ``device``: where the rectangles are computed (None: the GPU when there is one)."""
    from ..evaluation.coco_gt import load_json      # here, not at the top: evaluation imports data.catalog
    from ..structures.polygons import oriented_ratios

    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if isinstance(dataset_dicts_or_json, (list, tuple)):
        per_image = [d.get("annotations", []) for d in dataset_dicts_or_json]
    else:
        ds = load_json(dataset_dicts_or_json)
        pos = {im["id"]: i for i, im in enumerate(ds.get("images", []))}
        per_image = [[] for _ in pos]
        for ann in ds.get("annotations", []):
            if ann["image_id"] in pos:
                per_image[pos[ann["image_id"]]].append(ann)
    anns = list(itertools.chain.from_iterable(per_image))
    image_of = torch.tensor([i for i, a in enumerate(per_image) for _ in a], dtype=torch.int64)
    ratios = torch.from_numpy(oriented_ratios(anns, device))
    factors = torch.full((len(per_image),), 0.1, dtype=torch.float32)
    factors[image_of[ratios < 1 / 3].unique()] = 0.5
    factors[image_of[ratios < 1 / 5].unique()] = 1.0
    return factors


class TrainingSampler:
    """detectron2.data.samplers.TrainingSampler: an infinite stream of indices, every epoch a permutation of range(size) (or the
    range itself without ``shuffle``), of which rank r takes every world_size-th index starting at r."""

    def __init__(self, size, shuffle=True, seed=None, rank=0, world_size=1):
        if size <= 0:
            raise ValueError("TrainingSampler needs a positive size")
        self._size = int(size)
        self._shuffle = shuffle
        self._seed = _resolve_seed(seed, world_size)
        self._rank, self._world_size = int(rank), int(world_size)

    def __iter__(self):
        yield from itertools.islice(self._infinite_indices(), self._rank, None, self._world_size)

    def _infinite_indices(self):
        g = torch.Generator()
        g.manual_seed(self._seed)
        while True:
            if self._shuffle:
                yield from torch.randperm(self._size, generator=g).tolist()
            else:
                yield from range(self._size)


class RepeatFactorTrainingSampler:
    """detectron2.data.samplers.RepeatFactorTrainingSampler: per epoch, image i appears int(f_i) + (rand_i < frac(f_i)) times, with
    rand = torch.rand(len) from one seeded generator; the epoch's indices are then permuted by torch.randperm from the same generator
    (kept in order without ``shuffle``); rank r takes every world_size-th index of the infinite stream starting at r."""

    def __init__(self, repeat_factors, shuffle=True, seed=None, rank=0, world_size=1):
        repeat_factors = torch.as_tensor(repeat_factors, dtype=torch.float32)
        self._shuffle = shuffle
        self._seed = _resolve_seed(seed, world_size)
        self._rank, self._world_size = int(rank), int(world_size)
        self._int_part = torch.trunc(repeat_factors)
        self._frac_part = repeat_factors - self._int_part

    def _get_epoch_indices(self, generator):
        rands = torch.rand(len(self._frac_part), generator=generator)
        rep = self._int_part + (rands < self._frac_part).float()
        indices = []
        for i, r in enumerate(rep.tolist()):
            indices.extend([i] * int(r))
        return torch.tensor(indices, dtype=torch.int64)

    def __iter__(self):
        yield from itertools.islice(self._infinite_indices(), self._rank, None, self._world_size)

    def _infinite_indices(self):
        g = torch.Generator()
        g.manual_seed(self._seed)
        while True:
            indices = self._get_epoch_indices(g)
            if self._shuffle:
                yield from indices[torch.randperm(len(indices), generator=g)].tolist()
            else:
                yield from indices.tolist()


__all__ = ["RepeatFactorTrainingSampler", "TrainingSampler", "repeat_factors_from_ratios"]
