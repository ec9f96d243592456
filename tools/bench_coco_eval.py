"""Device time of a COCO-val-sized slender-object evaluation (slenderobjdet_amd.evaluation, csrc/coco_eval.hip).

A synthetic set from a seed: 5 000 images, 80 categories, gts as data/synthetic.py draws them, 100 scored detections per image
jittered from the gts.  Prints one JSON line: the device time of COCOEvaluator.evaluate_flat split into match (ordering + the
match kernel) / accumulate (ordering + the accumulate kernel) / ar (ordering + the recall pass), from events around a synchronise
after a warm-up; the kernel launches of one evaluation (torch profiler); the wall time of the whole evaluate including the host
summaries; and a hash of the output arrays.

    python tools/bench_coco_eval.py [--images 5000] [--cats 80] [--dets 100] [--iters 5] [--seed 0] [--rotated [--recall]]

``--rotated`` times RotatedCOCOEvaluator.evaluate_flat on ``synthetic_rotated_coco`` at the same size (match / accumulate phases;
the recall pass only with ``--recall``) and reports the share of the (detection, gt) pairs of the segments whose circumscribed circles meet, i.e.
that go on towards the polygon clipping.  ``--rotated --recall`` sets the metadata's ``rotated_recall``: the split then holds the
rotated recall pass as ``ar`` (ordering + sod_proposal_ar_rotated), with the minimum and maximum over the iterations beside the medians.
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slenderobjdet_amd.data.catalog import MetadataCatalog  # noqa: E402
from slenderobjdet_amd.evaluation import COCOEvaluator, RotatedCOCOEvaluator  # noqa: E402
from slenderobjdet_amd.evaluation.coco_evaluation import predictions_from_numpy  # noqa: E402
from slenderobjdet_amd.evaluation.synthetic import synthetic_coco, synthetic_rotated_coco  # noqa: E402


def _launches(ev, flat):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ev.evaluate_flat(flat)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type.name in ("CUDA", "PrivateUse1")]
        ours = [n for n in names if "coco" in n or "proposal_ar" in n]
        return len(names), len(ours)
    except Exception as e:  # noqa: BLE001 - the count is informative; the rocprofv3 run is the authoritative one
        print("profiler unavailable:", e, file=sys.stderr)
        return None, None


def _circle_share(ds, preds):
    """(pairs of the (image, category) segments, those whose circumscribed circles meet) - iou_rotated_impl's first early return."""
    cats = sorted(c["id"] for c in ds["categories"])
    gts = {}
    for a in ds["annotations"]:
        gts.setdefault(a["image_id"], []).append([cats.index(a["category_id"])] + list(a["bbox"][:4]))
    order = np.argsort(preds["image_id"], kind="stable")
    img_s = preds["image_id"][order]
    starts = np.flatnonzero(np.r_[True, img_s[1:] != img_s[:-1], True])
    pairs = near = 0
    for b, e in zip(starts[:-1], starts[1:]):
        g = np.array(gts.get(int(img_s[b]), []), np.float64).reshape(-1, 5)
        if not len(g):
            continue
        sel = order[b:e]
        d, c = preds["boxes"][sel].astype(np.float64), preds["category"][sel]
        same = c[:, None] == g[None, :, 0]
        rs = 0.5 * np.hypot(d[:, 2], d[:, 3])[:, None] + 0.5 * np.hypot(g[:, 3], g[:, 4])[None]
        d2 = (d[:, 0, None] - g[None, :, 1]) ** 2 + (d[:, 1, None] - g[None, :, 2]) ** 2
        pairs += int(same.sum())
        near += int((same & (d2 <= rs * rs * 1.0001)).sum())
    return pairs, near


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--cats", type=int, default=80)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--rotated", action="store_true", help="time the rotated-box evaluation (RotatedCOCOEvaluator)")
    ap.add_argument("--ratio-device", default=None,
                    help="take the gt ratios from structures.polygons.oriented_ratios on this device, through the metadata's ratio_device (COCOEvaluator only; default: the host loop)")
    ap.add_argument("--recall", action="store_true", help="with --rotated: add the rotated recall pass (metadata rotated_recall) and report it as 'ar'")
    a = ap.parse_args()
    if a.recall and not a.rotated:
        ap.error("--recall applies to --rotated (COCOEvaluator always runs its recall pass)")
    if a.rotated and a.ratio_device is not None:
        ap.error("--ratio-device applies to COCOEvaluator, not to --rotated")
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    synth = synthetic_rotated_coco if a.rotated else synthetic_coco
    ds, preds = synth(a.seed, n_images=a.images, n_cats=a.cats, dets_per_image=(a.dets, a.dets), no_dt=0.0)
    t_gen = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as tmp:
        jf = os.path.join(tmp, "gt.json")
        with open(jf, "w") as f:
            json.dump(ds, f)
        MetadataCatalog.get("bench_coco_eval").json_file = jf
        t0 = time.perf_counter()
        if a.ratio_device is not None:
            MetadataCatalog.get("bench_coco_eval").ratio_device = a.ratio_device
        if a.recall:
            MetadataCatalog.get("bench_coco_eval").rotated_recall = True
        ev = (RotatedCOCOEvaluator if a.rotated else COCOEvaluator)("bench_coco_eval", None, False)
        t_gt = time.perf_counter() - t0
    flat = predictions_from_numpy(preds, dev)
    ev.evaluate_flat(flat)          # warm-up: gt upload, scratch layout, code objects
    torch.cuda.synchronize()
    split = {"match": [], "accumulate": [], "ar": [], "total": []}
    wall = []
    for _ in range(a.iters):
        torch.cuda.synchronize()
        events = {}
        w0 = time.perf_counter()
        res = ev.evaluate_flat(flat, events=events)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - w0)
        e = {k: v[0] for k, v in events.items()}
        split["match"].append(e["match"].elapsed_time(e["accumulate"]))
        split["accumulate"].append(e["accumulate"].elapsed_time(e["end" if a.rotated else "ar"]))
        if not a.rotated:
            split["ar"].append(e["ar"].elapsed_time(e["end"]))
        elif a.recall:
            split["ar"].append(e["ar"].elapsed_time(e["ar_end"]))
        split["total"].append(e["match"].elapsed_time(e["ar_end" if a.recall else "end"]))
    h = hashlib.sha256()
    for arr in (ev.precision, ev.recall, ev.scores) + (() if a.rotated and not a.recall else (ev.recalls.numpy(),)):
        h.update(np.ascontiguousarray(arr).tobytes())
    n_all, n_ours = (None, None) if a.no_profile else _launches(ev, flat)
    out = {
        "metric": "coco_eval_device_ms", "images": a.images, "categories": a.cats, "detections": int(len(preds["score"])),
        "gts": len(ds["annotations"]),
        "device_ms": {k: round(float(np.median(v)), 3) for k, v in split.items() if v},
        "evaluate_wall_ms": round(float(np.median(wall)) * 1e3, 3),
        "gt_index_s": round(t_gt, 3), "synth_s": round(t_gen, 3),
        "kernel_launches": n_all, "coco_kernel_launches": n_ours,
        "AP": res["bbox"]["AP"], **({} if a.rotated else {"AR@100": res["ar"]["AR@100"]}), "output_sha256": h.hexdigest()[:16],
    }
    if a.recall:
        out["device_ms_min_max"] = {k: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in split.items() if v}
        out["AR@100"] = res["ar"]["AR@100"]
    if a.rotated:
        pairs, near = _circle_share(ds, preds)
        out.update(metric="rotated_coco_eval_device_ms", AR100=float(ev.stats[8] * 100), segment_pairs=pairs,
                   pairs_past_circle_test=near, share_past_circle_test=round(near / max(pairs, 1), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
