"""Test-time augmentation, the parts that need no GPU: the augmentation plan, the box round trip through the forward transform and the
restated un-mapping, the drop-in binding, the refusals and the input errors."""
import numpy as np
import pytest
import torch

import tta_restated as R
from slenderobjdet_amd.modeling import test_time_augmentation as TTA      # noqa: F401 - the feature under test: absent, nothing here can pass


def test_plan_basic():
    from slenderobjdet_amd.modeling.test_time_augmentation import tta_plan

    want = [(400, 533, False), (400, 533, True), (500, 667, False), (500, 667, True)]
    assert tta_plan(480, 640, (400, 500), 4000, True) == want
    assert R.plan(480, 640, (400, 500), 4000, True) == want


def test_plan_max_size_cap():
    from slenderobjdet_amd.modeling.test_time_augmentation import tta_plan

    assert tta_plan(100, 1000, (400,), 1333, False) == [(133, 1333, False)]
    assert R.plan(100, 1000, (400,), 1333, False) == [(133, 1333, False)]


def test_plan_no_flip_halves_the_list():
    from slenderobjdet_amd.config import fresh_cfg
    from slenderobjdet_amd.modeling.test_time_augmentation import DatasetMapperTTA, tta_plan

    sizes = (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
    both, plain = tta_plan(480, 640, sizes, 4000, True), tta_plan(480, 640, sizes, 4000, False)
    assert len(both) == 18 and len(plain) == 9
    assert plain == both[0::2] and all(not f for _, _, f in plain) and all(f for _, _, f in both[1::2])
    assert both == R.plan(480, 640, sizes, 4000, True)
    # the mapper object is the same plan from cfg.TEST.AUG (detectron2's defaults: 9 sizes, flip) and the shape of "image" as given
    assert DatasetMapperTTA(fresh_cfg())({"image": torch.zeros(3, 480, 640, dtype=torch.uint8), "height": 7, "width": 9}) == both


@pytest.mark.parametrize("flip", [False, True])
def test_round_trip_forward_transform_then_unmapping(flip):
    """transform_boxes (float32: scale = new / old rounded once, one product) forward, the restated un-mapping (float64) back: the
    forward side contributes two float32 roundings (scale and product) of a value up to max(side), the bound is 4 * 2^-22 * max(side)."""
    from slenderobjdet_amd.data.transforms import transform_boxes

    h, w, newh, neww = 37, 53, 61, 87
    g = torch.Generator().manual_seed(5)
    x = torch.rand(200, 2, generator=g).sort(dim=1).values * w
    y = torch.rand(200, 2, generator=g).sort(dim=1).values * h
    boxes = torch.stack((x[:, 0], y[:, 0], x[:, 1], y[:, 1]), 1)
    fwd = transform_boxes(boxes, h, w, newh, neww, flip)
    back, _, _, valid = R.unmap(fwd.numpy(), np.ones(200), np.zeros(200), (newh, neww), flip, (h, w), 1e-8)
    assert valid.all()
    bound = 4 * 2.0 ** -22 * max(h, w, newh, neww)
    assert np.abs(back - boxes.double().numpy()).max() <= bound


def _cpu_cfg(*args, **kw):
    from bench import make_cfg

    cfg = make_cfg(*args, **kw)
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def test_dropin_binds_the_stub_until_asked():
    import slenderobjdet_amd.dropin as dropin
    import detectron2.modeling as d2m
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.modeling.test_time_augmentation import DatasetMapperTTA, GeneralizedRCNNWithTTA

    dropin.install()                                  # what the import alone binds
    with pytest.raises(NotImplementedError):
        d2m.GeneralizedRCNNWithTTA(None, None)
    try:
        cls = dropin.bind_tta()
        assert cls is GeneralizedRCNNWithTTA and d2m.GeneralizedRCNNWithTTA is GeneralizedRCNNWithTTA
        assert d2m.DatasetMapperTTA is DatasetMapperTTA
        cfg = _cpu_cfg(18)
        model = build_model(cfg)
        tta = d2m.GeneralizedRCNNWithTTA(cfg, model)
        assert isinstance(tta, torch.nn.Module) and tta.model is model and tta.batch_size == 3
        assert tta.nms_thresh == model.nms_thresh and tta.max_detections == cfg.TEST.DETECTIONS_PER_IMAGE
    finally:
        dropin.install()                              # leave the default binding for the other tests of the session
        del d2m.DatasetMapperTTA


def test_refusals_name_their_reason():
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.modeling.test_time_augmentation import GeneralizedRCNNWithTTA

    cfg = _cpu_cfg(18, arch="rrcnn")
    with pytest.raises(ValueError, match="rotated"):
        GeneralizedRCNNWithTTA(cfg, build_model(cfg))
    cfg.MODEL.META_ARCHITECTURE = "ProposalNetwork"
    with pytest.raises(ValueError, match="ProposalNetwork"):
        GeneralizedRCNNWithTTA(cfg, build_model(cfg))
    with pytest.raises(ValueError, match="not supported"):
        GeneralizedRCNNWithTTA(cfg, torch.nn.Linear(2, 2))


def test_input_errors():
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.modeling.test_time_augmentation import GeneralizedRCNNWithTTA

    cfg = _cpu_cfg(18)
    tta = GeneralizedRCNNWithTTA(cfg, build_model(cfg))
    with pytest.raises(ValueError, match="file_name"):
        tta([{"file_name": "a.jpg", "height": 4, "width": 4}])
    with pytest.raises(ValueError, match="uint8"):
        tta([{"image": torch.zeros(3, 8, 8)}])
    with pytest.raises(ValueError, match="uint8"):
        tta([{"image": torch.zeros(8, 8, 3, dtype=torch.uint8)}])
