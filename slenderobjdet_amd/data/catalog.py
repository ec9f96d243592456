"""detectron2's MetadataCatalog: per-dataset metadata (``json_file``, ``thing_classes``, ``thing_dataset_id_to_contiguous_id``,
...) by name, attribute access on a dict."""


class Metadata(dict):
    def __getattr__(self, k):
        if k in self:
            return self[k]
        raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


class MetadataCatalog:
    _d = {}

    @classmethod
    def get(cls, name):
        return cls._d.setdefault(name, Metadata(name=name, evaluator_type="coco"))
