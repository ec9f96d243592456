"""Minimum-area rectangles of a COCO-train-sized synthetic polygon set: the device path against the host paths.

    python tools/bench_polygon_geom.py [--anns 860000] [--host-anns 20000] [--out profiles/polygon_geom_bench.txt]

Point counts are drawn from 6..400 with mean about 25 (a geometric tail), the points as blobs of image size rounded to 2 decimals.
Reports: pack_polygons; min_area_rects on the GPU end to end (host-to-device copy + kernel + device-to-host copy); the kernel alone
from device events (median of 20 launches after warm-up); the numpy path of structures.polygons and the evaluator's host loop
(coco_gt.polygon_ratio) on a subset, extrapolated; the largest difference between the device's and the numpy path's side ratios, of
the device's and the host loop's least areas, and how many ratios differ from the host loop's (ties of equal area, see below).
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slenderobjdet_amd import _C  # noqa: E402
from slenderobjdet_amd.evaluation.coco_gt import min_area_rect_sides, polygon_ratio  # noqa: E402
from slenderobjdet_amd.structures.polygons import min_area_rects, pack_polygons  # noqa: E402


def synthetic_annotations(n_anns, seed=0):
    rs = np.random.RandomState(seed)
    counts = np.clip(6 + rs.geometric(1.0 / 20.0, n_anns) - 1, 6, 400)
    total = int(counts.sum())
    size = rs.rand(n_anns, 2) * (300, 300) + 4
    centre = rs.rand(n_anns, 2) * (640, 480)
    rep = np.repeat(np.arange(n_anns), counts)
    pts = np.round(centre[rep] + (rs.rand(total, 2) - 0.5) * size[rep], 2)
    off = np.zeros(n_anns + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    flat = pts.reshape(-1)
    return [{"id": i, "iscrowd": 0, "bbox": [0, 0, 1, 1], "segmentation": [flat[2 * off[i]:2 * off[i + 1]].tolist()]} for i in range(n_anns)], float(counts.mean())


def ratios(rect):
    w, h = rect[:, 2], rect[:, 3]
    return np.where(w * h == 0, 0.0, np.minimum(w, h) / np.maximum(np.maximum(w, h), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anns", type=int, default=860000)
    ap.add_argument("--host-anns", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    anns, mean_pts = synthetic_annotations(a.anns, a.seed)
    t0 = time.perf_counter()
    xy, off, index = pack_polygons(anns)
    t_pack = time.perf_counter() - t0
    min_area_rects(xy[:off[64]], off[:65], dev)         # warm-up: library load, code object
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rect, info = min_area_rects(xy, off, dev)
    t_dev = time.perf_counter() - t0
    # the kernel alone
    A = len(off) - 1
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev)
    d_rect, d_info = torch.empty((A, 5), dtype=torch.float64, device=dev), torch.empty(A, dtype=torch.int32, device=dev)
    launch = lambda: _C.call("sod_polygon_min_area_rect", _C.ptr(d_xy), _C.ptr(d_off), A, _C.ptr(d_rect), _C.ptr(d_info), _C.stream_ptr())  # noqa: E731
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    same_as_api = bool(np.array_equal(d_rect.cpu().numpy(), rect))
    # host paths on a subset
    m = min(a.host_anns, A)
    t0 = time.perf_counter()
    rect_np, info_np = min_area_rects(xy[:off[m]], off[:m + 1], "cpu")
    t_np = time.perf_counter() - t0
    k = min(m, 5000)
    t0 = time.perf_counter()
    loop = np.array([polygon_ratio(x["segmentation"]) for x in anns[:k]])
    t_loop = time.perf_counter() - t0
    # equal areas of different directions (every acute triangle) are legitimate: the host loop resolves them by rounding noise, the
    # kernel by the first edge, so ratios may differ there while the least area cannot
    area_loop = np.array([np.prod(min_area_rect_sides(xy[off[i]:off[i + 1]])) for i in range(k)])
    area_rel = np.abs(rect[:k, 2] * rect[:k, 3] - area_loop) / area_loop
    out = {
        "metric": "polygon_min_area_rect", "annotations": A, "points": int(len(xy)), "mean_points": round(mean_pts, 2),
        "pack_s": round(t_pack, 3), "device_h2d_kernel_d2h_s": round(t_dev, 4), "pack_plus_device_s": round(t_pack + t_dev, 3),
        "kernel_ms_median20": round(float(np.median(ms)), 3), "kernel_ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
        "kernel_launch_equals_api_result": same_as_api,
        "numpy_path_subset": m, "numpy_path_s": round(t_np, 3), "numpy_path_extrapolated_s": round(t_np / m * A, 1),
        "host_loop_subset": k, "host_loop_s": round(t_loop, 3), "host_loop_extrapolated_s": round(t_loop / k * A, 1),
        "max_ratio_diff_device_vs_numpy": float(np.abs(ratios(rect[:m]) - ratios(rect_np)).max()),
        "max_rel_area_diff_device_vs_host_loop": float(area_rel.max()),
        "ratios_differing_from_host_loop_above_1e-9": int((np.abs(ratios(rect[:k]) - loop) > 1e-9).sum()),
        "degenerate": int((info < 3).sum()), "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
