"""Test-time augmentation (modeling/test_time_augmentation.py) on one card: a synthetic 480 x 640 uint8 image, the ``TEST.AUG`` defaults
(9 shortest-edge sizes 400 .. 1200, each with and without flip = 18 runs), FCOS R50-FPN and the axis-aligned Faster R-CNN R50-FPN from
random initialisation (thresholds lowered so that the runs return detections; their counts are printed with the figures):
  * ms per image of the whole wrapper (resize / flip on the device, 18 runs in groups of ``--batch-size``, merge, NMS);
  * us of the merge stage alone (``sod_tta_merge_candidates``, one launch);
  * us of the same merge written with torch ops on the device (per run: un-flip, scale, clip, threshold, pack);
  * ms of the 18 runs fed one by one through plain ``model([...])`` on images resized beforehand - what the code could do without
    the prepared-batch entry and the wrapper (no merge, no final NMS included).
Device events, warm-up, best of 3 blocks; prints the card's shader clock with the figures.

    python tools/bench_tta.py [--reps 5] [--batch-size 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import device_fingerprint, make_cfg  # noqa: E402
from slenderobjdet_amd.layers import functional as HF  # noqa: E402
from slenderobjdet_amd.modeling import build_model  # noqa: E402
from slenderobjdet_amd.modeling.test_time_augmentation import SCORE_THRESH, GeneralizedRCNNWithTTA  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch-size", type=int, default=3)
ap.add_argument("--fcos-thresh", type=float, default=0.005, help="MODEL.FCOS.INFERENCE_TH (random init: class scores sit at the 0.01 prior)")
ap.add_argument("--rcnn-thresh", type=float, default=0.0124, help="MODEL.ROI_HEADS.SCORE_THRESH_TEST (random init: probabilities about 1 / 81)")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
H, W = 480, 640


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record(); torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) / reps)
    return best


def cfg_of(arch):
    if arch == "fcos":
        cfg = make_cfg(50)
        cfg.MODEL.FCOS.INFERENCE_TH = args.fcos_thresh
        return cfg
    cfg = make_cfg(50, "rrcnn")          # the two-stage R50-FPN geometry, then back to axis-aligned boxes
    cfg.MODEL.PROPOSAL_GENERATOR.NAME, cfg.MODEL.ANCHOR_GENERATOR.NAME = "RPN", "DefaultAnchorGenerator"
    cfg.MODEL.ANCHOR_GENERATOR.ANGLES = [[-90, 0, 90]]
    cfg.MODEL.RPN.BBOX_REG_WEIGHTS = (1.0, 1.0, 1.0, 1.0)
    cfg.MODEL.ROI_HEADS.NAME, cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "StandardROIHeads", "ROIAlignV2"
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = args.rcnn_thresh
    return cfg


def merge_torch(dets, plan, height, width, D):
    """tta_merge_candidates with torch ops: the same padded candidate layout, one run at a time."""
    A = len(plan)
    boxes = torch.zeros((1, A * D, 4), dtype=torch.float32, device=dev)
    scores = torch.full((1, A * D), float("-inf"), dtype=torch.float32, device=dev)
    classes = torch.zeros((1, A * D), dtype=torch.int32, device=dev)
    for a, ((b, s, c), (h, w, flip)) in enumerate(zip(dets, plan)):
        n = s.shape[0]
        if n == 0:
            continue
        b = b.clone()
        if flip:
            b[:, 0], b[:, 2] = w - b[:, 2], w - b[:, 0].clone()
        b[:, 0::2] *= width / w
        b[:, 1::2] *= height / h
        b[:, 0::2].clamp_(0, width)
        b[:, 1::2].clamp_(0, height)
        ok = torch.isfinite(b).all(1) & torch.isfinite(s) & (s > SCORE_THRESH)
        sl = slice(a * D, a * D + n)
        boxes[0, sl] = torch.where(ok[:, None], b, torch.zeros_like(b))
        scores[0, sl] = torch.where(ok, s, torch.full_like(s, float("-inf")))
        classes[0, sl] = torch.where(ok, c.to(torch.int32), torch.zeros_like(c, dtype=torch.int32))
    return boxes, scores, classes


out = {"image": [H, W], "batch_size": args.batch_size, "device": device_fingerprint(0)}
g = torch.Generator().manual_seed(0)
image = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g).to(dev)
for arch in ("fcos", "rcnn"):
    cfg = cfg_of(arch)
    torch.manual_seed(0)
    model = build_model(cfg)
    model.eval()
    tta = GeneralizedRCNNWithTTA(cfg, model, batch_size=args.batch_size)
    plan = tta.tta_mapper({"image": image})
    inp = {"image": image, "height": H, "width": W}
    with torch.no_grad():
        final = tta([inp])[0]["instances"]
        t_all = timed(lambda: tta([inp]), args.reps)
        dets = tta._run_model(image.permute(1, 2, 0).contiguous(), plan)
        counts = [int(d[1].shape[0]) for d in dets]
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        D = max(max(counts), 1)
        cat_b = torch.cat([d[0] for d in dets]).float().contiguous()
        cat_s = torch.cat([d[1] for d in dets]).float().contiguous()
        cat_c = torch.cat([d[2] for d in dets]).to(torch.int32).contiguous()
        runs = [(0, a, h, w, f) for a, (h, w, f) in enumerate(plan)]
        t_merge = timed(lambda: HF.tta_merge_candidates(cat_b, cat_s, cat_c, off, runs, [(H, W)], len(plan), D, SCORE_THRESH), 50)
        t_torch = timed(lambda: merge_torch(dets, plan, H, W, D), 20)
        kb, ks, kc = HF.tta_merge_candidates(cat_b, cat_s, cat_c, off, runs, [(H, W)], len(plan), D, SCORE_THRESH)
        tb, ts, tc = merge_torch(dets, plan, H, W, D)
        same = bool(torch.equal(ks, ts) and torch.equal(kc, tc) and (kb - tb).abs().max().item() <= 4 * 2.0 ** -22 * 1600)
        # the 18 augmented images resized beforehand (outside the timing), fed one by one through the plain entry point
        pre = []
        for h, w, flip in plan:
            im = torch.nn.functional.interpolate(image[None].float(), size=(h, w), mode="bilinear", align_corners=False)[0]
            pre.append({"image": (im.flip(2) if flip else im).round().clamp(0, 255).to(torch.uint8).contiguous(), "height": h, "width": w})
        t_plain = timed(lambda: [model([p]) for p in pre], args.reps)
    out[arch] = {"runs": len(plan), "detections_per_run": counts, "final_detections": len(final), "wrapper_ms_per_image": round(t_all, 2),
                 "merge_kernel_us": round(t_merge * 1e3, 1), "merge_torch_ops_us": round(t_torch * 1e3, 1), "merge_outputs_agree": same,
                 "plain_runs_one_by_one_ms": round(t_plain, 2)}
    print(f"{arch}: wrapper {t_all:8.2f} ms/image | merge kernel {t_merge * 1e3:7.1f} us | merge with torch ops {t_torch * 1e3:8.1f} us "
          f"(outputs agree: {same}) | {len(plan)} plain runs one by one {t_plain:8.2f} ms | detections per run {counts}, final {len(final)}", flush=True)
    del model, tta
    torch.cuda.empty_cache()
out["device_after"] = device_fingerprint(0, clocks_only=True)
print(json.dumps(out))
