"""RotatedRetinaNet beside RetinaNet and the rotated R-CNN at equal settings (batch 16, 1333 x 800 images, R50-FPN, bf16 product path,
synthetic batches, bench.train_step with prefetch and the reference's warm-up schedule), one card:
  * us per call of ``sod_retina_label_rotated`` (N = 16, R = 22 400 * 18 = 403 200 anchors, G <= 50 per image) against the per-image
    composition of the existing entry points it replaces (``sod_anchor_match_rotated`` + ``sod_box2box_get_deltas`` + the class mapping),
    on the same inputs, the two alternating; the labels of the two are compared first;
  * img/s of a full training step of the three classes, built one after the other in this process.
Device events, warm-up, >= 20 timed calls; prints the card's shader clock with the figures.
``--box-loss rotated_iou`` / ``rotated_giou`` / ``rotated_kld`` trains RotatedRetinaNet's box regression with the rotated IoU / GIoU /
Gaussian KL-divergence loss (MODEL.RETINANET.BBOX_REG_LOSS_TYPE) instead of smooth-L1; ``--rotated-only`` times RotatedRetinaNet's step
alone (alternating runs of the box losses, one process each).  ``--box-kernels`` adds us per call of the box-loss kernels of the three
decoded-box losses, the entry points alternating: the pair operators ``sod_rotated_{iou,giou,kld}_loss`` (forward, forward + backward;
P = the step's 886 positives, 65 536 and 1 048 576 pairs) and the fused ``sod_retina_{riou,rgiou,rkld}_loss_{fwd,bwd}`` on the step's own
geometry (N * R = 16 * 403 200 anchors, the labeller's labels and matched boxes).

    python tools/bench_rotated_retinanet.py [--steps 20] [--warmup 5] [--skip-step] [--box-loss smooth_l1|rotated_iou|rotated_giou|rotated_kld]
                                            [--rotated-only] [--box-kernels] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import damp_residual_branches, device_fingerprint, make_cfg, train_step  # noqa: E402
from slenderobjdet_amd.data import SyntheticCocoBatches, synthetic_batch  # noqa: E402
from slenderobjdet_amd.layers import functional as HF  # noqa: E402
from slenderobjdet_amd.modeling import build_model  # noqa: E402
from slenderobjdet_amd.modeling.anchor_generator import grid_anchors_rotated  # noqa: E402
from slenderobjdet_amd.solver import build_lr_scheduler, build_optimizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="timed calls per round of the labelling comparison (three rounds)")
ap.add_argument("--skip-step", action="store_true", help="only the labelling comparison")
ap.add_argument("--box-loss", choices=["smooth_l1", "rotated_iou", "rotated_giou", "rotated_kld"], default="smooth_l1", help="RotatedRetinaNet's box regression loss")
ap.add_argument("--box-kernels", action="store_true", help="also time the pair operators and the fused kernels of the decoded-box losses")
ap.add_argument("--rotated-only", action="store_true", help="time RotatedRetinaNet's training step only, not the two other classes")
ap.add_argument("--out", default=None, help="also write the JSON result to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_rotated_retinanet: needs a GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
N, H, W, K = 16, 800, 1333, 80
strides = [8, 16, 32, 64, 128]
SIZES, RATIOS, ANGLES = [[32], [64], [128], [256], [512]], [[1.0, 2.0, 5.0]], [[-90, -60, -30, 0, 30, 60]]
W5 = (1.0, 1.0, 1.0, 1.0, 1.0)
THR, LAB = [0.4, 0.5], [0, -1, 1]
Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32        # the RetinaNet backbone's size divisibility: 800 x 1344, 22 400 locations
level_hw = [((Hp + s - 1) // s, (Wp + s - 1) // s) for s in strides]


def rotated_retina_cfg():
    cfg = make_cfg(50, "retinanet")
    cfg.MODEL.META_ARCHITECTURE = "RotatedRetinaNet"
    ag = cfg.MODEL.ANCHOR_GENERATOR
    ag.NAME, ag.SIZES, ag.ASPECT_RATIOS, ag.ANGLES = "RotatedAnchorGenerator", SIZES, RATIOS, ANGLES
    cfg.MODEL.RETINANET.BBOX_REG_WEIGHTS = W5
    cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = args.box_loss
    return cfg


assert sum(h * w for h, w in level_hw) == 22400
out = {"geometry": {"batch": N, "padded": [Hp, Wp], "level_hw": level_hw}, "device": device_fingerprint(0), "box_loss": args.box_loss}

# ---------------------------------------------------------------------------------------------- labelling
anchors = torch.cat(grid_anchors_rotated(level_hw, strides, SIZES, RATIOS, ANGLES, 0.0, dev)).contiguous()
R = anchors.shape[0]
data = synthetic_batch(N, H, W, 1234, device="cuda", rotated=True)
gts = [d["instances"].gt_boxes.tensor.float().contiguous() for d in data]
cls = [d["instances"].gt_classes.to(torch.int32).contiguous() for d in data]
counts = [len(g) for g in gts]
Gmax = max(counts)
pb, pc = torch.zeros(N, Gmax, 5, device=dev), torch.zeros(N, Gmax, dtype=torch.int32, device=dev)
for i in range(N):
    pb[i, : counts[i]], pc[i, : counts[i]] = gts[i], cls[i]
cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
ws = torch.empty(N * Gmax, dtype=torch.int32, device=dev)


def fused():
    return HF.retina_label_rotated(anchors, pb, pc, cnt, THR, LAB, True, K, W5, ws=ws)


labels_c = torch.empty(N, R, dtype=torch.int32, device=dev)
deltas_c = torch.empty(N, R, 5, device=dev)


def composed():
    """What a per-image label_anchors costs with the existing entry points: 2 match launches + the delta launch + the mapping."""
    for i in range(N):
        _, idx, ml = HF.anchor_match(gts[i], anchors, THR, LAB, True)
        il = idx.long()
        deltas_c[i] = HF.box2box_get_deltas(anchors, gts[i][il], W5)
        l = cls[i][il]
        labels_c[i] = torch.where(ml == 0, K, torch.where(ml == -1, -1, l))
    return labels_c, deltas_c


lab_f, d_f = fused()
lab_c, d_c = composed()
torch.cuda.synchronize()
pos = (lab_c >= 0) & (lab_c != K)
same = bool(torch.equal(lab_f, lab_c))
dmax = float((d_f[pos] - d_c[pos]).abs().max()) if int(pos.sum()) else 0.0


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3        # us per call


for _ in range(3):
    fused(); composed()
torch.cuda.synchronize()
tf, tc = [], []
for _ in range(3):                                # the two alternate: three windows each of --calls calls
    tf.append(window(fused, args.calls))
    tc.append(window(composed, args.calls))
out["labelling"] = {"N": N, "R": R, "gts": int(sum(counts)), "Gmax": Gmax, "labels_equal": same, "positives": int(pos.sum()),
                    "max_delta_difference": dmax, "calls_per_window": args.calls,
                    "sod_retina_label_rotated_us": [round(t, 1) for t in tf], "per_image_composition_us": [round(t, 1) for t in tc],
                    "sod_retina_label_rotated_mean_us": round(sum(tf) / len(tf), 1), "per_image_composition_mean_us": round(sum(tc) / len(tc), 1),
                    "launches": {"fused": 2, "composition_kernels": 3 * N}}
print(f"labelling N = {N}, R = {R}, {sum(counts)} gts (max {Gmax}): fused {sum(tf) / 3:8.1f} us {[round(t, 1) for t in tf]} | per-image composition "
      f"{sum(tc) / 3:8.1f} us {[round(t, 1) for t in tc]} | labels equal: {same}, {int(pos.sum())} positives, max delta difference {dmax:.3g}", flush=True)

# ---------------------------------------------------------------------------------------------- box-loss kernels
if args.box_kernels:
    g = torch.Generator().manual_seed(2)
    kt = {}

    def alternate(entries, calls):
        for fn in entries.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in entries}
        for _ in range(3):
            for k, fn in entries.items():
                t[k].append(window(fn, calls))
        for k, v in t.items():
            kt[k] = [round(x, 1) for x in v]
            print(f"  {k:44s} {sum(v) / len(v):9.1f} us  {[round(x, 1) for x in v]}", flush=True)

    for P in (886, 65536, 1048576):
        gt = torch.cat([16 + 1200 * torch.rand(P, 2, generator=g), 8 + 200 * torch.rand(P, 1, generator=g), 4 + 40 * torch.rand(P, 1, generator=g),
                        360 * torch.rand(P, 1, generator=g) - 180], 1)
        pr = gt + torch.cat([4 * torch.randn(P, 2, generator=g), 6 * torch.randn(P, 2, generator=g).abs(), 8 * torch.randn(P, 1, generator=g)], 1)
        pr, gt = pr.to(dev), gt.to(dev)
        entries = {}
        for stem in ("iou", "giou", "kld"):
            fwd, bwd = getattr(HF, f"rotated_{stem}_loss_fwd"), getattr(HF, f"rotated_{stem}_loss_bwd")
            entries[f"rotated_{stem}_loss fwd P={P}"] = lambda fwd=fwd: fwd(pr, gt)
            entries[f"rotated_{stem}_loss fwd+bwd P={P}"] = lambda fwd=fwd, bwd=bwd: (fwd(pr, gt), bwd(pr, gt))
        print(f"pair operators, P = {P}, three windows of {args.calls} calls:", flush=True)
        alternate(entries, args.calls)
    lab_b, mb = HF.retina_label_rotated(anchors, pb, pc, cnt, THR, LAB, True, K, W5, ws=ws, want_boxes=True)
    A = R // sum(h * w for h, w in level_hw)
    pitch = (A * 5 + 7) // 8 * 8
    pred = (0.1 * torch.randn(N, R // A, pitch, generator=g)).to(dev)
    dpred = torch.empty(N, R // A, pitch, dtype=HF.ACT_DTYPE, device=dev)
    nrm, one = torch.full((1,), 100.0, device=dev), torch.ones(1, device=dev)
    entries = {}
    for stem in ("riou", "rgiou", "rkld"):
        fwd, bwd = getattr(HF, f"retina_{stem}_loss_fwd"), getattr(HF, f"retina_{stem}_loss_bwd")
        entries[f"retina_{stem}_loss_fwd"] = lambda fwd=fwd: fwd(pred, pitch, lab_b, anchors, mb, N, R, A, K, W5, 4.135166556742356, nrm, 1.0)
        entries[f"retina_{stem}_loss_bwd"] = lambda bwd=bwd: bwd(pred, pitch, lab_b, anchors, mb, N, R, A, K, W5, 4.135166556742356, one, nrm, dpred)
    print(f"fused kernels, N * R = {N} * {R}, A = {A}, pitch {pitch}, {int(((lab_b >= 0) & (lab_b != K)).sum())} positives:", flush=True)
    alternate(entries, args.calls)
    out["box_kernels_us"] = kt

# ---------------------------------------------------------------------------------------------- training steps
if not args.skip_step:
    classes = (("RotatedRetinaNet", rotated_retina_cfg(), True), ("RetinaNet", make_cfg(50, "retinanet"), False),
               ("GeneralizedRCNN+RRPN+RROIHeads", make_cfg(50, "rrcnn"), True))
    for arch, cfg, rotated in classes[:1] if args.rotated_only else classes:
        torch.manual_seed(1)
        model = build_model(cfg)
        model.train()
        damp_residual_branches(model)      # random-init R50 without a checkpoint overflows the un-normalised heads (bench.py)
        opt = build_optimizer(cfg, model)
        sched = build_lr_scheduler(cfg, opt)
        loader = SyntheticCocoBatches(N, H, W, rank=0, device=dev, pool=2, rotated=rotated)
        cur = next(loader)
        for _ in range(args.warmup):
            nxt = next(loader)
            train_step(model, opt, cur, nxt, sched)
            cur = nxt
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.steps):
            nxt = next(loader)
            total = train_step(model, opt, cur, nxt, sched)
            cur = nxt
        e.record(); torch.cuda.synchronize()
        ips = N * args.steps / (s.elapsed_time(e) * 1e-3)
        out[arch] = {"img_per_s": round(ips, 1), "steps": args.steps, "warmup": args.warmup, "last_total_loss": round(float(total), 4)}
        print(f"{arch}: {ips:7.1f} img/s over {args.steps} steps (last total loss {float(total):.4f})", flush=True)
        del model, opt, sched, loader
        torch.cuda.empty_cache()
out["device_after"] = device_fingerprint(0, clocks_only=True)
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
