"""FCOSRepPoints beside FCOSV2 and RepPointsDetector at equal settings (batch 16, 1333 x 800 images, five levels, synthetic gts, R50-FPN,
bf16 product path, bench.train_step with prefetch), one card:
  * us per call of the entry points the model adds: ``sod_fcos_assign_topk`` plain and slender (radius 1.5), ``sod_fcos_rpd_refine_targets``
    for the batch against the N calls of ``sod_anchor_match`` it replaces, ``sod_points2ltrb_fwd`` over the five levels;
  * img/s of a full training step of the three classes.
Device events, warm-up, >= 20 repetitions; prints the card's shader clock with the figures.

    python tools/bench_fcos_reppoints.py [--steps 20] [--skip-step]
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
ap.add_argument("--skip-step", action="store_true", help="only the entry points")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
N, H, W = 16, 800, 1333
strides = [8, 16, 32, 64, 128]
Hp, Wp = (H + 127) // 128 * 128, (W + 127) // 128 * 128
level_hw = [((Hp + s - 1) // s, (Wp + s - 1) // s) for s in strides]
L = sum(h * w for h, w in level_hw)


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
t_p = timed(lambda: HF.fcos_assign_topk(boxes, classes, offs, N, level_hw, strides, SIZES_OF_INTEREST, 1.5, 80, 5))
t_s = timed(lambda: HF.fcos_assign_topk(boxes, classes, offs, N, level_hw, strides, SIZES_OF_INTEREST, 1.5, 80, 5, slender=True))
# candidates: boxes of 1-3 strides around every location
g = torch.Generator().manual_seed(0)
st = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(level_hw, strides)])
loc = torch.cat([torch.stack((((torch.arange(w) * s + s // 2).float()[None].expand(h, w)).reshape(-1),
                              ((torch.arange(h) * s + s // 2).float()[:, None].expand(h, w)).reshape(-1)), 1) for (h, w), s in zip(level_hw, strides)])
d = (torch.rand(N, L, 4, generator=g) * 2 + 1) * st[None, :, None]
cand = torch.stack([loc[None, :, 0] - d[..., 0], loc[None, :, 1] - d[..., 1], loc[None, :, 0] + d[..., 2], loc[None, :, 1] + d[..., 3]], 2).contiguous().to(dev)
image_hw = torch.tensor([[float(H), float(W)]] * N).to(dev)
t_b = timed(lambda: HF.fcos_rpd_refine_targets(boxes, classes, offs, counts, cand, image_hw, level_hw, strides, 80, [0.4, 0.5], [0, -1, 1], True))


def per_image():
    b0 = 0
    for i, c in enumerate(counts):
        HF.anchor_match(boxes[b0:b0 + c], cand[i], [0.4, 0.5], [0, -1, 1], True)
        b0 += c


t_n = timed(per_image)
pts = [torch.randn(N, h, w, 24, device=dev) for h, w in level_hw]
ltrb, bx, arg = torch.empty(N, L, 4, device=dev), torch.empty(N, L, 4, device=dev), torch.empty(N, L, dtype=torch.int32, device=dev)


def p2l():
    o = 0
    for l, (h, w) in enumerate(level_hw):
        HF.points2ltrb_fwd(pts[l], None, strides[l], 2 ** l, 9, ltrb.view(-1)[o * 4:], bx.view(-1)[o * 4:], L * 4, arg.view(-1)[o:], L)
        o += h * w


t_l = timed(p2l)
out["entry_points_us"] = {"sod_fcos_assign_topk": round(t_p * 1e3, 1), "sod_fcos_assign_topk_slender": round(t_s * 1e3, 1),
                          "sod_fcos_rpd_refine_targets": round(t_b * 1e3, 1), "sod_anchor_match_x_N": round(t_n * 1e3, 1),
                          "sod_points2ltrb_fwd_x_5": round(t_l * 1e3, 1)}
print(f"assign_topk {t_p * 1e3:7.1f} us | slender {t_s * 1e3:7.1f} us | refine targets, batch {t_b * 1e3:7.1f} us | {N} x anchor_match {t_n * 1e3:7.1f} us | "
      f"points2ltrb x 5 {t_l * 1e3:7.1f} us | {sum(counts)} gts, L = {L}", flush=True)

if not args.skip_step:
    for arch, family in (("FCOSV2", "fcos"), ("RepPointsDetector", "reppoints"), ("FCOSRepPoints", "fcos")):
        cfg = make_cfg(50, family, constant_lr=True)
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
