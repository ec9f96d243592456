"""Minimum-area rectangles of polygons on the host: the numpy path of structures/polygons.py against the float64 restatement
(polygon_geom_restated.py), known answers, the degenerate rule, and the consumers that need no GPU - oriented_ratios, coco_to_rotated,
tools/mask_to_rbox.py, repeat_factors_from_ratios and the samplers."""
import importlib.util
import itertools
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import polygon_geom_restated as R

from slenderobjdet_amd.evaluation import coco_gt
from slenderobjdet_amd.evaluation.coco_gt import CocoGt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rects(point_sets, device="cpu"):
    from slenderobjdet_amd.structures import min_area_rects

    xy = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in point_sets])
    off = np.cumsum([0] + [len(np.asarray(p).reshape(-1, 2)) for p in point_sets])
    return min_area_rects(xy, off, device)


def rotated_rectangle(cx, cy, w, h, deg):
    """Corners of the rectangle whose width axis is (cos a, -sin a) and height axis (sin a, cos a)."""
    a = math.radians(deg)
    wx, wy, hx, hy = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    return [(cx + sx * w / 2 * wx + sy * h / 2 * hx, cy + sx * w / 2 * wy + sy * h / 2 * hy) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def test_abi_symbol_and_constants():
    from slenderobjdet_amd import _C
    from slenderobjdet_amd.structures import polygons

    header = open(os.path.join(ROOT, "include", "slender_hip.h")).read()
    assert re.search(r"\bint\s+sod_polygon_min_area_rect\s*\(", header)
    assert len(_C._SIGS["sod_polygon_min_area_rect"]) == 6
    defs = dict(re.findall(r"#define\s+(SOD_POLYGON_\w+)\s+(\(?[\w<> ]+\)?)", header))
    assert eval(defs["SOD_POLYGON_LDS_POINTS"]) == polygons.LDS_POINTS
    assert eval(defs["SOD_POLYGON_MAX_POINTS"]) == polygons.MAX_POINTS
    assert eval(defs["SOD_POLYGON_MAX_ANNS"]) == polygons.MAX_ANNS
    assert "polygon_geom.hip" in open(os.path.join(ROOT, "slenderobjdet_amd", "csrc", "Makefile")).read()


# a 60 x 20 rectangle turned by `deg`: the canonical (w, h, angle), quarter turns taken off by hand
KNOWN = [(-80, 20, 60, 10), (-45, 20, 60, 45), (-30, 60, 20, -30), (0, 60, 20, 0), (30, 60, 20, 30), (45, 60, 20, 45),
         (60, 20, 60, -30), (90, 20, 60, 0), (135, 20, 60, 45)]


@pytest.mark.parametrize("deg,w,h,a", KNOWN)
def test_known_rotated_rectangles(deg, w, h, a):
    rect, info = _rects([rotated_rectangle(123.5, 77.25, 60.0, 20.0, deg)])
    got = rect[0].copy()
    assert info[0] == 4 and -45.0 < got[4] <= 45.0
    if a == 45 and got[4] < 0:
        # the corners carry the rounding of cos / sin 45, so the edge's angle is 45 +- 1e-14 and may fold to the other end of
        # (-45, 45]: (h, w, -45 + tiny) is the same rectangle one tie-free rounding step away
        got[2], got[3], got[4] = got[3], got[2], got[4] + 90.0
    assert np.abs(got - np.array([123.5, 77.25, w, h, a])).max() <= 1e-9, (deg, rect[0])


def test_known_axis_aligned_rectangles():
    x0, y0, W, H = 10.5, 20.25, 80.0, 40.0
    four = [(x0, y0), (x0 + W, y0), (x0 + W, y0 + H), (x0, y0 + H)]
    closed = four + four[:1]
    forty = ([(x0 + 8 * i, y0) for i in range(10)] + [(x0 + W, y0 + 4 * i) for i in range(10)]
             + [(x0 + W - 8 * i, y0 + H) for i in range(10)] + [(x0, y0 + H - 4 * i) for i in range(10)])
    assert len(forty) == 40
    rect, info = _rects([four, closed, forty, four[::-1], four[2:] + four[:2]])
    for r in rect:
        assert r.tolist() == [x0 + W / 2, y0 + H / 2, W, H, 0.0] and not math.copysign(1, r[4]) < 0
    assert info.tolist() == [4] * 5


def test_degenerate_inputs_give_the_extent_box():
    line = [(0.5 * i, 0.25 * i + 1.0) for i in range(50)]                   # exactly representable, exactly collinear
    rs = np.random.RandomState(3)
    # 1e-13 of jitter ALONG an axis-parallel line: near-coincident distinct points, still exactly collinear
    jitter = [(float(i // 2) + 1e-13 * rs.rand(), 7.25) for i in range(50)]
    cases = [([(5.0, 7.0)] * 3, (5.0, 7.0, 0.0, 0.0), 1),
             ([(1.0, 2.0), (4.0, 6.0), (1.0, 2.0)], (2.5, 4.0, 3.0, 4.0), 2),
             (line, (12.25, 7.125, 24.5, 12.25), 2),
             (jitter, None, 2)]
    rect, info = _rects([c[0] for c in cases])
    for (pts, want, hull), r, i in zip(cases, rect, info):
        p = np.array(pts)
        if want is None:
            want = ((p[:, 0].min() + p[:, 0].max()) / 2, 7.25, p[:, 0].max() - p[:, 0].min(), 0.0)
        assert r.tolist() == [*want, 0.0], (r, want)
        assert i == hull and i < 3
        assert R.min_area_rect(p)[0] == tuple(r.tolist())


def test_jitter_across_a_line_follows_the_oracle():
    """1e-13 of jitter ACROSS a slanted line leaves points that are not collinear in float64: a hull of three or more vertices and a
    rectangle whose least area is rounding noise.  What the degenerate rule promises does not apply; the path has to return, enclose
    the points and agree with the oracle's area within the side tolerance."""
    rs = np.random.RandomState(4)
    pts = np.array([(i, 0.5 * i + 1e-13 * rs.rand()) for i in range(50)], np.float64)
    rect, info = _rects([pts])
    R.check_parity([pts], [R.min_area_rect(pts)], rect, info, cap=None)


def test_cpu_path_against_restatement():
    """2 000 generated annotations.  Left out of the five-number comparison by the oracle alone (ties of two directions, fold at 45):
    16 of 2 000 = 0.8 %, 13 triangles and 3 quadrilaterals."""
    from slenderobjdet_amd.structures import min_area_rects, pack_polygons

    polys, pts, oracle = R.generated_with_oracle(2000)
    xy, off, index = pack_polygons(R.as_annotations(polys))
    assert index.tolist() == list(range(2000)) and off[-1] == len(xy) == sum(len(p) for p in pts)
    rect, info = min_area_rects(xy, off, "cpu")
    assert info.dtype == np.int32
    left_out = R.check_parity(pts, oracle, rect, info)
    print("left out of the full comparison:", left_out)


def _inline_dataset():
    hexagon = [10.0, 10.0, 90.0, 14.0, 130.0, 40.0, 118.0, 71.0, 40.0, 80.0, 5.0, 45.0]
    sliver = [200.0, 200.0, 330.0, 262.0, 334.0, 270.0, 203.0, 208.0]
    cap = [300.0, 20.0, 340.0, 25.0, 350.0, 60.0, 310.0, 64.0, 290.0, 40.0]
    anns = [
        {"id": 1, "image_id": 1, "category_id": 1, "iscrowd": 0, "bbox": [5, 10, 125, 70], "segmentation": [hexagon]},
        {"id": 2, "image_id": 1, "category_id": 1, "iscrowd": 0, "bbox": [200, 200, 134, 70], "segmentation": [sliver[:4], sliver]},
        {"id": 3, "image_id": 1, "category_id": 2, "iscrowd": 0, "bbox": [290, 20, 60, 44], "segmentation": [cap, hexagon]},
        {"id": 4, "image_id": 2, "category_id": 1, "iscrowd": 1, "bbox": [10, 20, 30, 90], "segmentation": {"counts": [1, 2], "size": [4, 4]}},
        {"id": 5, "image_id": 2, "category_id": 1, "iscrowd": 1, "bbox": [10, 20, 80, 20], "segmentation": [hexagon]},
        {"id": 6, "image_id": 2, "category_id": 2, "iscrowd": 0, "bbox": [1, 2, 30, 40], "ratio": 0.125, "segmentation": [hexagon]},
        {"id": 7, "image_id": 2, "category_id": 2, "iscrowd": 0, "bbox": [1, 2, 50, 10]},
        {"id": 8, "image_id": 2, "category_id": 2, "iscrowd": 0, "bbox": [1, 2, 12, 48], "segmentation": [[1.0, 2.0, 13.0, 50.0]]},
        {"id": 9, "image_id": 2, "category_id": 1, "iscrowd": 0, "bbox": [0, 0, 9, 9], "segmentation": [[0.0, 0.0, 4.0, 4.0, 9.0, 9.0]]},
    ]
    return {"images": [{"id": 1, "width": 640, "height": 480}, {"id": 2, "width": 640, "height": 480}],
            "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}], "annotations": anns}


def test_usable_and_pack():
    from slenderobjdet_amd.structures import pack_polygons, usable_polygons

    anns = _inline_dataset()["annotations"]
    assert [len(usable_polygons(a)) for a in anns] == [1, 1, 2, 0, 1, 1, 0, 0, 1]
    xy, off, index = pack_polygons(anns)
    assert index.tolist() == [0, 1, 2, 5, 8] and index.dtype == np.int64          # crowds and polygon-less annotations stay out
    assert off.tolist() == [0, 6, 10, 21, 27, 30] and off.dtype == np.int32 and xy.shape == (30, 2) and xy.dtype == np.float64
    assert xy[6:10].reshape(-1).tolist() == anns[1]["segmentation"][1]
    xy, off, index = pack_polygons([])
    assert xy.shape == (0, 2) and off.tolist() == [0] and len(index) == 0


def test_oriented_ratios_equal_the_host_loop():
    from slenderobjdet_amd.structures import oriented_ratios

    ds = _inline_dataset()
    want = [coco_gt.gt_ratio(a) for a in ds["annotations"]]
    for a in ds["annotations"]:
        polys = [p for p in a["segmentation"] if len(p) >= 6] if isinstance(a.get("segmentation"), list) else []
        if polys:
            assert not R.is_tie(R.min_area_rect(R.points_of(polys))[2])                 # non-tie cases only
    got = oriented_ratios(ds["annotations"], "cpu")
    assert got.dtype == np.float64 and got.shape == (9,)
    assert np.abs(got - np.array(want)).max() <= 1e-9, (got, want)
    assert got[3] == 30 / 90 and got[4] == 20 / 80 and got[5] == 0.125 and got[6] == 10 / 50 and got[7] == 12 / 48
    assert got[8] == 1.0                                                                 # collinear points: the 9 x 9 extent box, as polygon_ratio
    assert 0 < got[1] < 0.1                                                              # the sliver is slender; its bbox is not
    gt = CocoGt(ds, ratio_device="cpu")
    assert np.array_equal(gt.ratios, got)
    assert np.abs(CocoGt(ds).ratios - got).max() <= 1e-9
    assert len(oriented_ratios([], "cpu")) == 0


def test_evaluator_takes_ratio_device_from_the_metadata(tmp_path):
    from slenderobjdet_amd.data.catalog import MetadataCatalog
    from slenderobjdet_amd.evaluation import COCOEvaluator
    from slenderobjdet_amd.structures import oriented_ratios

    ds = _inline_dataset()
    jf = tmp_path / "gt.json"
    jf.write_text(json.dumps(ds))
    meta = MetadataCatalog.get("polygon_geom_host_ratio_device")
    meta.clear()
    meta.update(name="polygon_geom_host_ratio_device", json_file=str(jf))
    default = COCOEvaluator("polygon_geom_host_ratio_device", None, False)._gt.ratios
    assert np.array_equal(default, CocoGt(ds).ratios)
    meta["ratio_device"] = "cpu"
    assert np.array_equal(COCOEvaluator("polygon_geom_host_ratio_device", None, False)._gt.ratios, oriented_ratios(ds["annotations"], "cpu"))


def _rect_dataset():
    rects = [(100.0, 100.0, 60.0, 20.0, 30.0), (300.0, 120.0, 40.0, 30.0, -20.0), (480.0, 300.0, 150.0, 30.0, -15.0),
             (200.0, 200.0, 24.0, 18.0, 0.0), (420.0, 90.0, 12.0, 90.0, 40.0)]
    anns = []
    for i, r in enumerate(rects):
        corners = rotated_rectangle(*r)
        xs, ys = [c[0] for c in corners], [c[1] for c in corners]
        anns.append({"id": i + 1, "image_id": 1 if i < 3 else 2, "category_id": 1, "iscrowd": 0, "area": r[2] * r[3],
                     "bbox": [min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)], "segmentation": [[v for c in corners for v in c]]})
    anns.append({"id": 6, "image_id": 2, "category_id": 1, "iscrowd": 1, "area": 1200.0, "bbox": [10, 20, 30, 40],
                 "segmentation": {"counts": [1, 2], "size": [4, 4]}})
    ds = {"images": [{"id": 1, "width": 640, "height": 480}, {"id": 2, "width": 640, "height": 480}],
          "categories": [{"id": 1, "name": "thing"}], "annotations": anns}
    return ds, rects


def test_coco_to_rotated():
    from slenderobjdet_amd.data import coco_to_rotated

    ds, rects = _rect_dataset()
    before = json.dumps(ds)
    kept = coco_to_rotated(ds, skip_crowd=False, device="cpu")
    assert json.dumps(ds) == before                                                      # the input is left alone
    assert [a["id"] for a in kept["annotations"]] == [1, 2, 3, 4, 5, 6]
    assert kept["annotations"][5]["bbox"] == [10, 20, 30, 40, 0]                         # compute_rbox: the corner stays, angle 0
    out = coco_to_rotated(ds, skip_crowd=True, device="cpu")
    assert [a["id"] for a in out["annotations"]] == [1, 2, 3, 4, 5]
    assert out["images"] == ds["images"] and out["categories"] == ds["categories"]
    assert isinstance(out["info"]["description"], str) and "otated" in out["info"]["description"]
    for a, r in zip(out["annotations"], rects):
        assert len(a["bbox"]) == 5 and all(type(v) is float for v in a["bbox"])
        assert np.abs(np.array(a["bbox"]) - np.array(r)).max() <= 1e-9
        assert a["segmentation"] == ds["annotations"][a["id"] - 1]["segmentation"] and a["area"] == r[2] * r[3]
    json.dumps(out)
    box5 = CocoGt(out).rotated_arrays()["seg_box5"]
    assert box5.dtype == np.float32 and np.abs(box5 - np.array(rects, np.float32)).max() <= 1e-4
    bad = json.loads(before)
    bad["annotations"][1]["segmentation"] = [[1.0, 2.0, 3.0, 4.0]]
    with pytest.raises(ValueError, match=r"annotation 2\b"):
        coco_to_rotated(bad, skip_crowd=True, device="cpu")
    del bad["annotations"][1]["segmentation"]
    with pytest.raises(ValueError, match=r"annotation 2\b"):
        coco_to_rotated(bad, skip_crowd=True, device="cpu")


def test_mask_to_rbox_tool_output_loads_in_the_rotated_evaluator(tmp_path):
    from slenderobjdet_amd.data.catalog import MetadataCatalog
    from slenderobjdet_amd.evaluation import RotatedCOCOEvaluator

    spec = importlib.util.spec_from_file_location("mask_to_rbox_tool", os.path.join(ROOT, "tools", "mask_to_rbox.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ds, rects = _rect_dataset()
    src, dst = tmp_path / "instances_val.json", tmp_path / "rbox_val.json"
    src.write_text(json.dumps(ds))
    tool.main([str(src), str(dst), "--device", "cpu"])                                    # "val" in the name: crowds are dropped
    out = json.loads(dst.read_text())
    assert [len(a["bbox"]) for a in out["annotations"]] == [5] * 5
    meta = MetadataCatalog.get("polygon_geom_rbox_tool")
    meta.clear()
    meta.update(name="polygon_geom_rbox_tool", json_file=str(dst))
    ev = RotatedCOCOEvaluator("polygon_geom_rbox_tool", None, False)
    assert np.abs(ev._gt.rotated_arrays()["seg_box5"] - np.array(rects, np.float32)).max() <= 1e-4
    tool.main([str(src), str(dst), "--device", "cpu", "--keep-crowd"])
    assert len(json.loads(dst.read_text())["annotations"]) == 6


def _box_ann(w, h, x0=10.0, y0=20.0):
    return {"iscrowd": 0, "bbox": [x0, y0, w, h], "segmentation": [[x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h]]}


def test_repeat_factors_from_ratios():
    from slenderobjdet_amd.data import repeat_factors_from_ratios

    images = [
        [_box_ann(100.0, 19.99)],                              # just below 1/5
        [_box_ann(100.0, 20.0)],                               # 1/5 itself is not below it
        [_box_ann(100.0, 20.01)],                              # just above 1/5
        [_box_ann(33.33, 100.0)],                              # just below 1/3
        [_box_ann(100.0, 33.34)],                              # just above 1/3
        [],
        [_box_ann(100.0, 90.0), _box_ann(100.0, 30.0), _box_ann(10.0, 100.0)],
        [_box_ann(10.0, 100.0), _box_ann(100.0, 30.0), _box_ann(100.0, 90.0)],           # the same, in the other order
        [{"iscrowd": 0, "bbox": [0, 0, 100, 50], "ratio": 0.1}],
        [{"iscrowd": 1, "bbox": [0, 0, 100, 25], "segmentation": {"counts": [], "size": [1, 1]}}],
    ]
    want = [1.0, 0.5, 0.5, 0.5, 0.1, 0.1, 1.0, 1.0, 1.0, 0.5]
    f = repeat_factors_from_ratios([{"annotations": a} for a in images], device="cpu")
    assert f.dtype == torch.float32 and f.tolist() == torch.tensor(want, dtype=torch.float32).tolist()
    coco = {"images": [{"id": 100 + i} for i in range(len(images))], "categories": [{"id": 1, "name": "a"}],
            "annotations": [dict(a, id=0, category_id=1, image_id=100 + i) for i in reversed(range(len(images))) for a in images[i]]}
    assert torch.equal(repeat_factors_from_ratios(coco, device="cpu"), f)


def _epochs(factors, seed, n):
    """The first n epochs of detectron2's rule, recomputed from the generator calls it makes."""
    g = torch.Generator()
    g.manual_seed(seed)
    f = torch.tensor(factors, dtype=torch.float32)
    out = []
    for _ in range(n):
        rands = torch.rand(len(f), generator=g)
        rep = torch.trunc(f) + (rands < f - torch.trunc(f)).float()
        idx = torch.tensor([i for i, r in enumerate(rep.tolist()) for _ in range(int(r))], dtype=torch.int64)
        out.append(idx[torch.randperm(len(idx), generator=g)].tolist())
    return out


def test_repeat_factor_sampler_follows_the_rule():
    from slenderobjdet_amd.data import RepeatFactorTrainingSampler

    factors = [0.1, 0.5, 1.0, 2.3, 0.5, 0.1, 1.0, 3.0, 0.75, 1.5] * 3
    epochs = _epochs(factors, 7, 3)
    total = sum(len(e) for e in epochs)
    stream = list(itertools.islice(iter(RepeatFactorTrainingSampler(torch.tensor(factors), seed=7)), total))
    pos = 0
    for e in epochs:
        assert sorted(stream[pos:pos + len(e)]) == sorted(e)         # the multiset of the int + (rand < frac) rule
        assert stream[pos:pos + len(e)] == e                         # and the permutation from the same generator
        pos += len(e)
        counts = np.bincount(e, minlength=len(factors))
        assert all(int(f) <= c <= int(f) + 1 for f, c in zip(factors, counts))
    # ranks partition the stream
    parts = [list(itertools.islice(iter(RepeatFactorTrainingSampler(factors, seed=7, rank=r, world_size=3)), 40)) for r in range(3)]
    merged = [parts[i % 3][i // 3] for i in range(120)]
    assert merged == list(itertools.islice(iter(RepeatFactorTrainingSampler(factors, seed=7)), 120))
    with pytest.raises(ValueError):
        RepeatFactorTrainingSampler(factors, rank=0, world_size=2)      # several ranks must share a seed


def test_repeat_factor_presence_rate():
    """50 images of factor 0.1 and a last one of factor 1, which closes every unshuffled epoch: over 200 epochs the 10 000 draws
    are Bernoulli(0.1); 4 sigma = 4 * sqrt(10 000 * 0.1 * 0.9) = 120."""
    from slenderobjdet_amd.data import RepeatFactorTrainingSampler

    it = iter(RepeatFactorTrainingSampler([0.1] * 50 + [1.0], shuffle=False, seed=11))
    seen = epochs = 0
    per_image = np.zeros(50, np.int64)
    while epochs < 200:
        i = next(it)
        if i == 50:
            epochs += 1
        else:
            seen += 1
            per_image[i] += 1
    assert abs(seen - 1000) <= 120, seen
    assert per_image.max() <= 200 and per_image.min() >= 1


def test_training_sampler():
    from slenderobjdet_amd.data import TrainingSampler

    s = list(itertools.islice(iter(TrainingSampler(10, seed=3)), 30))
    assert all(sorted(s[i:i + 10]) == list(range(10)) for i in (0, 10, 20)) and s[:10] != s[10:20]
    g = torch.Generator()
    g.manual_seed(3)
    assert s[:10] == torch.randperm(10, generator=g).tolist()
    assert list(itertools.islice(iter(TrainingSampler(4, shuffle=False, seed=0)), 9)) == [0, 1, 2, 3, 0, 1, 2, 3, 0]
    parts = [list(itertools.islice(iter(TrainingSampler(10, seed=3, rank=r, world_size=2)), 15)) for r in range(2)]
    assert [parts[i % 2][i // 2] for i in range(30)] == s


def test_min_area_rects_refuses_bad_offsets():
    from slenderobjdet_amd.structures import min_area_rects

    xy = np.zeros((4, 2))
    for off in ([0, 3], [1, 4], [0, 2, 2, 4], [0, 3, 2, 4], []):
        with pytest.raises(ValueError):
            min_area_rects(xy, off, "cpu")
    rect, info = min_area_rects(np.zeros((0, 2)), [0], "cpu")
    assert rect.shape == (0, 5) and info.shape == (0,)
