"""FCOSTopK against FCOS at the headline geometry (batch 16, 1333 x 800 images, five levels, synthetic gts), one card:
  * us per call of ``sod_fcos_assign`` and of ``sod_fcos_assign_topk`` (assignment + gt index, the per-gt selection pass, three sums);
  * img/s of a full training step of ``FCOS`` and of ``FCOSTopK`` (R50-FPN, bf16 product path, bench.train_step with prefetch).
Device events, warm-up, >= 20 repetitions; prints the card's shader clock with the figures.

    python tools/bench_fcos_topk.py [--steps 20] [--skip-step]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import device_fingerprint, make_cfg, train_step  # noqa: E402
from slenderobjdet_amd.data import SyntheticCocoBatches, synthetic_batch  # noqa: E402
from slenderobjdet_amd.layers import functional as HF  # noqa: E402
from slenderobjdet_amd.modeling import build_model  # noqa: E402
from slenderobjdet_amd.modeling.meta_arch.fcos import SIZES_OF_INTEREST  # noqa: E402
from slenderobjdet_amd.solver import build_optimizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--skip-step", action="store_true", help="only the two assignment entry points")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
N, H, W = 16, 800, 1333
strides = [8, 16, 32, 64, 128]
Hp, Wp = (H + 127) // 128 * 128, (W + 127) // 128 * 128
level_hw = [((Hp + s - 1) // s, (Wp + s - 1) // s) for s in strides]


def timed(fn, reps=20):
    for _ in range(3):
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


out = {"geometry": {"batch": N, "padded": [Hp, Wp], "level_hw": level_hw}, "device": device_fingerprint(0)}
data = synthetic_batch(N, H, W, 1234, device="cuda")
counts = [len(d["instances"]) for d in data]
boxes = torch.cat([d["instances"].gt_boxes.tensor for d in data]).float().contiguous()
classes = torch.cat([d["instances"].gt_classes for d in data]).to(torch.int32).contiguous()
offs = torch.tensor([0] + counts).cumsum(0).to(torch.int32).to(dev)
out["gts"] = int(sum(counts))
for radius in (1.5, 0.0):
    t_a = timed(lambda: HF.fcos_assign(boxes, classes, offs, N, level_hw, strides, SIZES_OF_INTEREST, radius, 80))
    t_k = timed(lambda: HF.fcos_assign_topk(boxes, classes, offs, N, level_hw, strides, SIZES_OF_INTEREST, radius, 80, 5))
    r = HF.fcos_assign_topk(boxes, classes, offs, N, level_hw, strides, SIZES_OF_INTEREST, radius, 80, 5)
    out[f"radius_{radius}"] = {"sod_fcos_assign_us": round(t_a * 1e3, 1), "sod_fcos_assign_topk_us": round(t_k * 1e3, 1),
                               "positives": int(r[5][0]), "selected": int(r[4].sum())}
    print(f"radius {radius}: sod_fcos_assign {t_a * 1e3:7.1f} us | sod_fcos_assign_topk {t_k * 1e3:7.1f} us | {int(r[5][0])} positives, "
          f"{int(r[4].sum())} selected, {sum(counts)} gts", flush=True)

if not args.skip_step:
    for arch in ("FCOS", "FCOSTopK"):
        cfg = make_cfg(50, "fcos", constant_lr=True)
        cfg.MODEL.META_ARCHITECTURE = arch
        torch.manual_seed(0)
        model = build_model(cfg)
        model.train()
        opt = build_optimizer(cfg, model)
        loader = SyntheticCocoBatches(N, H, W, rank=0, device=dev, pool=2)
        cur = next(loader)
        for _ in range(args.warmup):
            nxt = next(loader)
            train_step(model, opt, cur, nxt)
            cur = nxt
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.steps):
            nxt = next(loader)
            total = train_step(model, opt, cur, nxt)
            cur = nxt
        e.record(); torch.cuda.synchronize()
        ips = N * args.steps / (s.elapsed_time(e) * 1e-3)
        out[arch] = {"img_per_s": round(ips, 1), "steps": args.steps, "last_total_loss": round(float(total), 4)}
        print(f"{arch}: {ips:7.1f} img/s over {args.steps} steps (last total loss {float(total):.4f})", flush=True)
        del model, opt, loader
        torch.cuda.empty_cache()
out["device_after"] = device_fingerprint(0, clocks_only=True)
print(json.dumps(out))
