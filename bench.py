#!/usr/bin/env python
"""Headline benchmark: training img/s of FCOS R50-FPN (FCOSV2, giou, center sampling 1.5 — the semantics of the
reference's configs/fcos/fcos_R_50_FPN_1x.yaml) on synthetic COCO-shaped 1333x800 batches, bf16 compute, 16 images per
GPU, one process per GPU (RCCL data parallel when launched under torch.distributed.run).

A step = forward + backward (gradient all-reduce when N>1) + fused SGD step on one resident synthetic batch.
Prints ONE JSON line on rank 0 (see the task contract).  A plain run sets up, warms up, times --steps steps and prints
the line, nothing else.  --full adds what takes runs or steps of its own: `roofline` (dominant conv kernel, measured
with HIP events recorded on the launch stream during sampled timed steps), `cpu_baseline` (the CPU oracle timed on a
bounded sample: it is test infrastructure and only ever the thing timed beside the product, never part of it), the
host-side probes (enqueue lead, three un-timed steps into empty queues) and the device fingerprint.

--dump-outputs DIR writes what the last timed step hands its caller, as float32 .npy files (snapshot_outputs): its
losses and a fixed, seeded sample of the parameters it updated.  Inputs and initial weights are seeded, so two builds
run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0   # dense bf16, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense"
HBM_ACHIEVABLE_GBPS = 6300.0   # what a streaming kernel sustains on MI355X (MI355X_MICROARCH.md; 8 TB/s is the spec figure)
TRAIN_FLOP_PER_IMAGE = 1.1913e12   # fwd + dgrad + wgrad, stem+res2 frozen, 800x1344


ARCH_NAMES = {"fcos": "FCOS", "retinanet": "RetinaNet", "reppoints": "RepPoints", "rrcnn": "rotated Faster R-CNN"}


def make_cfg(depth=50, arch="fcos", constant_lr=False):
    """BASELINE.json configs[1] (fcos, the headline), configs[2] (retinanet) and configs[3] (reppoints) as config objects.  ``BASE_LR`` is the
    reference configuration's; ``constant_lr`` (a run WITHOUT the reference's warm-up schedule, bench.py --constant-lr) lowers it to 0.002
    for the two architectures that diverge from random initialisation at their full rate."""
    from slenderobjdet_amd.config import fresh_cfg

    cfg = fresh_cfg()
    cfg.MODEL.META_ARCHITECTURE = "FCOSV2"
    cfg.MODEL.BACKBONE.NAME = "build_retinanet_resnet_fpn_backbone_use_p5"
    cfg.MODEL.RESNETS.OUT_FEATURES = ["res3", "res4", "res5"]
    cfg.MODEL.FPN.IN_FEATURES = ["res3", "res4", "res5"]
    cfg.MODEL.RESNETS.DEPTH = depth
    if depth in (18, 34):
        cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 64
    cfg.SOLVER.BASE_LR = 0.01                    # the architectures below lower it where random initialisation needs that
    if arch in ("retinanet", "reppoints"):      # configs/retina/Base-RetinaNet.yaml
        cfg.MODEL.BACKBONE.NAME = "build_retinanet_resnet_fpn_backbone"
        cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)] for x in [32, 64, 128, 256, 512]]
        cfg.MODEL.RETINANET.IOU_THRESHOLDS = [0.4, 0.5]
        cfg.MODEL.RETINANET.IOU_LABELS = [0, -1, 1]
        cfg.MODEL.META_ARCHITECTURE = "RetinaNet"
    if arch == "rrcnn":                          # configs/rotated/faster_R_101.yaml over Base-RRCNN-FPN.yaml
        cfg.MODEL.META_ARCHITECTURE = "GeneralizedRCNN"
        cfg.MODEL.BACKBONE.NAME = "build_resnet_fpn_backbone"
        cfg.MODEL.RESNETS.OUT_FEATURES = ["res2", "res3", "res4", "res5"]
        cfg.MODEL.FPN.IN_FEATURES = ["res2", "res3", "res4", "res5"]
        cfg.MODEL.PROPOSAL_GENERATOR.NAME = "RRPN"
        cfg.MODEL.ANCHOR_GENERATOR.NAME = "RotatedAnchorGenerator"
        cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[32], [64], [128], [256], [512]]
        cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS = [[0.5, 1.0, 2.0]]
        cfg.MODEL.ANCHOR_GENERATOR.ANGLES = [[45, 0, -45]]
        cfg.MODEL.RPN.HEAD_NAME = "StandardRPNHead"
        cfg.MODEL.RPN.BBOX_REG_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0)
        cfg.MODEL.RPN.IN_FEATURES = ["p2", "p3", "p4", "p5", "p6"]
        cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.PRE_NMS_TOPK_TEST = 2000, 1000
        cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TEST = 1000, 1000
        cfg.MODEL.ROI_HEADS.NAME = "RROIHeads"
        cfg.MODEL.ROI_HEADS.IN_FEATURES = ["p2", "p3", "p4", "p5"]
        cfg.MODEL.ROI_BOX_HEAD.NAME = "FastRCNNConvFCHead"
        cfg.MODEL.ROI_BOX_HEAD.NUM_FC = 2
        cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION = 7
        cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "ROIAlignRotated"
        cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS = (10.0, 5.0, 5.0, 5.0, 1.0)
        cfg.SOLVER.BASE_LR = 0.02       # configs/rotated/Base-RRCNN-FPN.yaml; without the warm-up schedule random init diverges there
        if constant_lr:
            cfg.SOLVER.BASE_LR = 0.002
    if arch == "reppoints":                      # configs/rep-points/rep_points_detector_R_50_FPN_1x.yaml
        cfg.MODEL.META_ARCHITECTURE = "RepPointsDetector"
        cfg.MODEL.RESNETS.OUT_FEATURES = ["res2", "res3", "res4", "res5"]
        cfg.MODEL.FPN.IN_FEATURES = ["res2", "res3", "res4", "res5"]
        cfg.MODEL.FPN.NORM = "GN"
        cfg.MODEL.PROPOSAL_GENERATOR.SAMPLE_MODE = "points"
        # The reference starts from an ImageNet checkpoint and warms up from 1e-3 x BASE_LR (0.01) over 1000 iterations: bench.py steps that
        # schedule since round 5.  At a CONSTANT 0.01 from random initialisation the run diverges within ~40 steps (loss 19 -> 70) and the
        # learned offsets leave the DeformConv kernels' LDS windows (431 img/s over steps 5-14, 413 over 7-36, 340 over 9-48): --constant-lr
        # therefore runs at 0.002.
        if constant_lr:
            cfg.SOLVER.BASE_LR = 0.002
    cfg.MODEL.FCOS.CENTER_SAMPLING_RADIUS = 1.5
    cfg.MODEL.FCOS.IOU_LOSS_TYPE = "giou"
    cfg.MODEL.FCOS.CENTERNESS_ON_REG = True
    cfg.SOLVER.IMS_PER_BATCH = 16
    return cfg


WORKLOADS = {
    "fcos": "FCOS R50-FPN (FCOSV2, giou, center-sampling 1.5), fwd+bwd+SGD, synthetic 1333x800 padded to 800x1344 (BASELINE.json configs[1])",
    "retinanet": "RetinaNet R50-FPN (9 anchors, smooth-L1), fwd+bwd+SGD, synthetic 1333x800 padded to 800x1344 (BASELINE.json configs[2])",
    "rrcnn": "GeneralizedRCNN + RRPN + RROIHeads (rotated boxes, ROIAlignRotated, rotated NMS), fwd+bwd+SGD, synthetic 1333x800 padded to 800x1344 "
             "(BASELINE.json configs[4])",
    "reppoints": "RepPointsDetector R50-FPN(GN) (points matcher, 2 DeformConv/level), fwd+bwd+SGD, synthetic 1333x800 padded to 800x1344 "
                 "(BASELINE.json configs[3])",
}


def damp_residual_branches(model, gamma=0.25):
    """Random-init ResNet-50 with identity FrozenBN doubles the activation variance in every residual block (x256 in std over 16
    blocks); the reference never sees that because it starts from an ImageNet checkpoint.  FCOS / RepPoints survive it (GroupNorm
    in the head / FPN), RetinaNet's un-normalised head overflows (loss_cls 7.5e6 at step 0, NaN at step 1).  With no checkpoint
    available, the RetinaNet benchmark sets the last FrozenBN weight of every block to ``gamma`` — the same kernels and FLOPs, sane
    numerics."""
    n = 0
    with torch.no_grad():
        for name, m in model.named_modules():
            if name.endswith(".conv3") and getattr(m, "frozen_bn", False):
                m.bn_weight.fill_(gamma)
                n += 1
            if name.endswith("stem.conv1") and getattr(m, "frozen_bn", False):
                m.bn_weight.fill_(1.0 / 64)     # pixel-range inputs (PIXEL_STD = 1): a trained stem BN brings them to O(1)
                n += 1
    return n


# SOD_PREFETCH=0: no software pipelining of the frozen backbone prefix (see train_step).  The next batch's prefix is enqueued between this
# step's forward and backward.  (Round 5 also measured it at the END of backward - started when the main stream has finished its data
# gradients, beside the weight-gradient tail, the optimizer and the next step's prologue: 640.0 vs 642.9 img/s, three alternating 100-step
# pairs; the weight-gradient tail is the critical path there and the prefix's whole-CU workgroups lengthen it.)
PREFETCH = os.environ.get("SOD_PREFETCH", "1") != "0"


def train_step(model, optimizer, data, next_data=None, scheduler=None, losses_out=None):
    """One training step.  ``next_data`` (optional) is the batch of the FOLLOWING step: between this step's forward and backward the
    model runs that batch's preprocess + frozen stem/res2 on a side stream (meta-arch ``prefetch``), where the HBM-bound frozen convs
    share the GPU with the MFMA-bound head backward; the next step's forward picks the result up.  Every step still carries exactly one
    frozen prefix (the next batch's instead of its own).  ``losses_out`` (a dict, optional) receives the step's loss tensors."""
    losses = model(data)
    if losses_out is not None:
        losses_out.clear()
        losses_out.update(losses)
    if next_data is not None and PREFETCH and hasattr(model, "prefetch"):
        model.prefetch(next_data)
    total = sum(losses.values())
    optimizer.zero_grad()
    model.arena.begin_backward()
    total.backward()
    model.arena.finish_backward()
    optimizer.step()
    if scheduler is not None:       # the reference steps its WarmupMultiStepLR once per iteration (detectron2 hooks.LRScheduler.after_step)
        scheduler.step()
    return total


def variant_kernel_name(code, mode=0):
    """sod_conv_last_variant() code -> the kernel name rocprofv3 prints (slender_hip.h)."""
    if code == 256:
        return f"void sodconv::conv_igemm256_kernel<{mode}, false>"
    bq, bp, bk = code // 100000, (code // 100) % 1000, code % 100
    generic, bk = bk & 1, bk & ~1
    wq, wp, fq, fp = {(16, 256): (1, 4, 1, 4), (64, 256): (1, 4, 4, 4), (128, 128): (2, 2, 4, 4), (128, 256): (2, 4, 4, 4)}.get((bq, bp), (0, 0, 0, 0))
    return f"void conv_igemm_kernel<{mode}, {'true' if generic else 'false'}, {wq}, {wp}, {fq}, {fp}, false, {bk}, "


KIND_MODE = {"conv_fwd": 0, "conv_dgrad": 1, "conv_wgrad": 2}


def kernel_name(kind, code):
    """(kind, sod_conv_prof_collect variant code) -> the kernel name rocprofv3 prints."""
    if code == -7:
        return "stem_fused_kernel"
    if code == -8:
        return "bottleneck_frozen_kernel"
    if code == 7003:            # conv_ws3.hip: persistent weight-stationary 3x3 kernel (128 -> 128 channels)
        return "void sodconv::conv_ws3_kernel<" + ("0" if kind == "conv_fwd" else "1")
    if code == 7001:            # conv_pw.hip: persistent weight-stationary kernel of the expanding 1x1 convolutions
        return "void sodconv::conv_pw_kernel<" + ("0" if kind == "conv_fwd" else "1")
    if kind == "conv_wgrad":
        if code == 256:
            return "sodconv::conv_wgrad256_kernel"
        if code == 9009:             # conv_wgrad9.hip: the nine taps of a 3x3 convolution in one workgroup
            return "sodconv::conv_wgrad9_kernel"
        if code == 32004:            # conv_wgrad_fold.hip: taps folded into the tile rows (few output channels)
            return "sodconv::conv_wgrad_fold_kernel"
        if 1000 <= code < 3000:      # conv_wgrad_ring.hip: G*1000 + NSTAGE*100 + EPI*10 -> conv_wgrad_ring_kernel<G, NSTAGE, EPI, ABL = 0>
            return f"conv_wgrad_ring_kernel<{code // 1000}, {(code // 100) % 10}, {(code // 10) % 10}, 0>"
        return f"void conv_wgrad_kernel<{code // 1000}, {code % 1000}>"
    return variant_kernel_name(code, KIND_MODE[kind])


def algo_bytes(kind, desc):
    """ALGORITHMIC HBM bytes of one conv dispatch: every operand of the convolution read or written exactly once (bf16 activations and
    weights, the fp32 weight gradient written once); fused epilogue operands (residual, ReLU mask, accumulate) are not counted."""
    if not desc:
        return 0.0
    if desc[0] == "ml":
        _, N, hs, C, K, R, stride, ws = desc[:8]
        hw = list(zip(hs, ws))
    else:
        N, H, W, C, K, R, stride = desc[:7]
        if R == "bneck":      # fused frozen bottleneck block: x in, 256-channel block output out, four weight matrices
            return N * H * W * (C + K) * 2.0 + (C * 64 + 64 * 64 * 9 + 64 * K + (C * K if C != K else 0)) * 2.0
        if R == 7 and C == 3:      # fused stem: uint8 RGB in, pooled 64-channel bf16 out
            return N * H * W * 3.0 + N * (H // 4) * (W // 4) * K * 2.0 + K * 49 * 8 * 2.0
        hw = [(H, W)]
    act = sum(N * h * w * C + N * -(-h // stride) * -(-w // stride) * K for h, w in hw) * 2.0
    return act + K * R * R * C * (4.0 if kind == "conv_wgrad" else 2.0)


def fused_bytes(kind, desc):
    """algo_bytes + the operands of the epilogue FUSED into the launch, each once: the shortcut a bottleneck's conv3 adds, the gradient of
    the identity path a data gradient accumulates, the ReLU mask (tensor or 1 bit per element) it applies or writes.  These bytes belong
    to the operator the launch implements (the reference runs them as separate elementwise kernels: conv -> add -> relu), so THIS is the
    byte count an HBM-bound launch must be priced against; `hbm_frac` (convolution operands only) is kept beside it for continuity."""
    extra = desc[7] if desc and desc[0] != "ml" and len(desc) > 7 and not isinstance(desc[5], str) else 0
    return algo_bytes(kind, desc) + float(extra)


def roofline_report(prof, prof_steps, args):
    """`roofline` = the conv kernel with the most GPU time in the sampled steps (duration = hipEvent interval on its launch
    stream, algorithmic FLOPs = 2*N*Ho*Wo*K*R*S*C with UN-padded channel counts); every other kernel in `kernels`;
    `backbone_convs` = ResNet body + FPN, the convolutions north_star's >= 0.5 x MFMA target is stated for; `head_convs` = the rest."""
    by_k, groups, kinds = {}, {}, {}
    for kind, flops, sec, desc, variant in prof:
        for tab, key in ((by_k, (kind, variant)), (kinds, kind), (groups, "head_convs" if desc and desc[0] == "ml" else "backbone_convs")):
            a = tab.setdefault(key, [0.0, 0.0, 0, 0.0, 0.0])
            a[0] += flops; a[1] += sec; a[2] += 1; a[3] += algo_bytes(kind, desc); a[4] += fused_bytes(kind, desc)

    def row(v, name=None):
        # frac = share of the dense MFMA peak; hbm_frac = ALGORITHMIC bytes (every conv operand once) / time / the achievable HBM rate;
        # bound = the roof this group of launches sits closer to (a 1x1 convolution at frac 0.2 and hbm_frac 0.5 is an HBM-bound kernel at
        # half its roof, not an MFMA kernel at a fifth of it)
        fl, sec, cnt, nbytes, fbytes = v[:5]
        mf, hf, ff = fl / sec / 1e12 / MFMA_PEAK_TFLOPS, nbytes / sec / 1e9 / HBM_ACHIEVABLE_GBPS, fbytes / sec / 1e9 / HBM_ACHIEVABLE_GBPS
        r = {"TFLOP/s": round(fl / sec / 1e12, 2), "frac": round(mf, 4), "hbm_GBps_algorithmic": round(nbytes / sec / 1e9, 1), "hbm_frac": round(hf, 4),
             "hbm_frac_fused": round(ff, 4),      # incl. the fused epilogue operands (shortcut / accumulate / mask), each once: fused_bytes()
             "bound": "mfma" if mf >= ff else "hbm", "ms_per_step": round(sec / prof_steps * 1e3, 3),
             "launches_per_step": round(cnt / prof_steps, 1), "tflop_per_step": round(fl / prof_steps / 1e12, 3),
             # the floor the bytes set: time of these launches if every fused byte moved once at the achievable HBM rate, and the MFMA
             # fraction the group would show at that floor - the distance of an HBM-bound group to north_star's 0.5 as a number
             "byte_floor_ms_per_step": round(fbytes / prof_steps / (HBM_ACHIEVABLE_GBPS * 1e9) * 1e3, 3),
             "frac_at_byte_floor": round(fl / (fbytes / (HBM_ACHIEVABLE_GBPS * 1e9)) / 1e12 / MFMA_PEAK_TFLOPS, 4) if fbytes else None}
        if name:
            r["kernel"] = name
        return r

    dom = max(by_k, key=lambda k: by_k[k][1])
    fl, sec, cnt, nbytes = by_k[dom][:4]
    kname = kernel_name(*dom)
    tr = pmc_traffic(dom[0], kname, args.arch)
    rep = {"bound": "mfma", "kernel": kname, "achieved": round(fl / sec / 1e12, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
           "frac": round(fl / sec / 1e12 / MFMA_PEAK_TFLOPS, 4), "traffic": (tr or {}).get("hbm_bytes_per_launch"),
           "traffic_source": (tr or {}).get("source"),
           "algorithmic_bytes": round(nbytes / cnt), "algorithmic_bytes_note": "per launch, conv operands read / written once (no fused epilogue operands)",
           "traffic_over_algorithmic": round(tr["hbm_bytes_per_launch"] / (nbytes / cnt), 3) if tr and nbytes else None,
           "hbm_GBps_algorithmic": round(nbytes / sec / 1e9, 1), "hbm_frac": round(nbytes / sec / 1e9 / HBM_ACHIEVABLE_GBPS, 4),
           "selection": "kernel with the largest share of conv GPU time in the sampled steps", "launches": cnt, "sampled_steps": prof_steps,
           "avg_launch_us": round(sec / cnt * 1e6, 2), "ms_per_step": round(sec / prof_steps * 1e3, 3),
           "flops": "algorithmic, un-padded channels",
           "sampling": f"{prof_steps} of the {args.steps} timed steps (every 32nd from step K/2; all with --dump-prof); sampled steps run the weight gradients and the box tower on the main stream so that every interval is one kernel's duration",
           "kernels": [row(v, kernel_name(*k)) for k, v in sorted(by_k.items(), key=lambda kv: -kv[1][1])],
           "by_pass": {k: row(v) for k, v in kinds.items()}}
    if args.arch == "fcos":
        for gname, v in groups.items():
            rep[gname] = row(v)
    st = pmc_step_traffic(args.arch)
    if st:
        rep["step_hbm"] = st
    return rep


def pmc_files(arch):
    """The committed PMC summaries of ``arch``, oldest to newest by tag: the headline's are profiles/<tag>_pmc.json (r1b < r2a < ... < r6a), the
    other architectures' profiles/<tag>_<arch>_pmc.json (tools/profile_arch.sh)."""
    import glob
    import re

    pat = re.compile(r"^r\d+[a-z]?_pmc\.json$" if arch == "fcos" else r"^r\d+[a-z]?_%s_pmc\.json$" % re.escape(arch))
    return sorted((f for f in glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json")) if pat.match(os.path.basename(f))), key=os.path.basename)


def pmc_step_traffic(arch="fcos"):
    """HBM bytes of one whole training step from the newest committed PMC summary (every kernel's FETCH_SIZE x 2 + WRITE_SIZE times its
    launches, divided by the steps of that profiled run): with the step time of THAT run it gives the step-level HBM rate the verdict
    of round 4 computed by hand (2.5 TB/s = 0.40 of the achievable rate).  None if no summary is committed."""
    files = pmc_files(arch)
    if not files:
        return None
    try:
        d = json.load(open(files[-1]))
        steps = int(d.get("steps", 7))
        tot = sum(k["hbm_bytes_per_launch"] * k["launches"] for k in d["kernels"].values()) / steps
        out = {"bytes_per_step": round(tot), "source": os.path.relpath(files[-1], ROOT), "profiled_steps": steps}
        if d.get("ms_per_step"):
            out["hbm_GBps"] = round(tot / (d["ms_per_step"] * 1e-3) / 1e9, 1)
            out["hbm_frac"] = round(out["hbm_GBps"] / HBM_ACHIEVABLE_GBPS, 4)
        return out
    except Exception:
        return None


def pmc_traffic(kind, kernel_name_, arch="fcos"):
    """HBM bytes per launch of a kernel from the newest committed rocprofv3 PMC summary (profiles/*_pmc.json: separate --pmc
    FETCH_SIZE / WRITE_SIZE runs of this same command, FETCH_SIZE doubled per MI355X_MICROARCH.md).  None if absent."""
    def norm(x):
        return x.replace(";", ",").replace(" ", "").replace("void", "")

    # by NAME (tags are ordered: r1b < r2a < ... < r3a): modification times are all equal in a fresh checkout
    files = pmc_files(arch)
    if not files:
        return None
    try:
        kernels = json.load(open(files[-1]))["kernels"]
        want = norm(kernel_name_)
        hits = [(v["launches"], k, v) for k, v in kernels.items() if want in norm(k)]
        if not hits:
            return None
        _, name, k = max(hits)
        return {"hbm_bytes_per_launch": k["hbm_bytes_per_launch"], "kernel": name, "source": os.path.relpath(files[-1], ROOT)}
    except Exception:
        return None


def usable_cpus():
    """CPUs this process may actually use: the affinity mask, cut down to the cgroup's CPU quota when there is one (a one-GPU box is a
    16-CPU share of a 256-CPU host; torch sized by the host's count runs the CPU baseline on an over-subscribed pool)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]           # cgroup v2
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period) + 0.5)))
    except Exception:      # noqa: BLE001
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())               # cgroup v1
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and p > 0:
                n = min(n, max(1, int(q / p + 0.5)))
        except Exception:      # noqa: BLE001
            pass
    return n


def cpu_baseline(model, args):
    """Time the CPU oracle (oracle/{model,reppoints,rcnn}.py) on a bounded sample of the same workload, host cores of this box.  SURVEY.md
    §8(d) asks for 3 warm-up + 10 timed iterations: that is the default (``--cpu-warmup`` / ``--cpu-steps``) whenever it fits; a 16-image
    CPU step takes ~20 s, so the sample is bounded to ``--cpu-images`` (2) images per step - about 35 s in all for FCOS - and, for the
    architectures whose oracle has Python-loop operators (DeformConv, rotated ROIAlign), to as many steps as fit ~45 s (at least 1 + 2);
    `sample` says what was run.  The two-stage oracle takes its sampled anchors / proposals from one forward pass of the product on the
    same images (subsampling is random; the oracle pins it, tests/test_gpu_rcnn.py): proposal selection + NMS are not in its timed step."""
    from slenderobjdet_amd.data import synthetic_batch

    cores = min(usable_cpus(), args.cpu_threads)   # more threads than this only adds oneDNN scheduling overhead
    torch.set_num_threads(cores)
    n = args.cpu_images
    rotated = args.arch == "rrcnn"
    data = synthetic_batch(n, 800, 1333, 4321, device="cpu", rotated=rotated)
    extra, note = (), ""
    if args.arch == "fcos":
        from oracle.model import OracleFCOS as Oracle
    elif args.arch == "retinanet":
        from oracle.model import OracleRetinaNet as Oracle
    elif args.arch == "reppoints":
        from oracle.reppoints import OracleRepPoints as Oracle
    else:
        from oracle.rcnn import OracleRCNN as Oracle
        gpu_data = [{"image": d["image"].cuda(), "instances": d["instances"].to("cuda")} for d in data]
        with torch.no_grad():
            model(gpu_data)
        rpn_labels, _m, rpn_deltas = (t.cpu() for t in model.proposal_generator.last_targets)
        props = model.roi_heads.last_proposals
        # The ROI heads on a SUBSET of the sampled proposals: with random-init weights the proposals are map-sized, the adaptive sampling grid
        # of ROIAlign(Rotated) then has ~1 000 samples per bin, and even the vectorised CPU restatement (oracle/detection.py:roi_align_vec;
        # the parity tests' Python-loop form needs minutes per ROI level) spends ~0.3 s per ROI: 2 x 512 proposals would be a 10-minute step.
        keep = 32                                    # proposals per image that reach the ROI heads on the CPU
        from oracle import detection as _od
        _od.ROI_ALIGN_IMPL = "vec"
        rois = torch.cat([torch.cat((torch.full((min(len(p), keep), 1), float(i)), p.proposal_boxes.tensor.cpu()[:keep]), 1) for i, p in enumerate(props)])
        extra = (rpn_labels, rpn_deltas, rois, torch.cat([p.gt_classes.cpu()[:keep] for p in props]), torch.cat([p.gt_boxes.tensor.cpu()[:keep] for p in props]))
        note = (f" (sampled anchors taken from one product forward on the same images; ROI heads on the first {keep} of the "
                f"{max(len(p) for p in props)} sampled proposals per image - a LOWER bound of the CPU's work, i.e. an upper bound of its rate: "
                "proposal selection, NMS and 15/16 of ROIAlign + box head are not in the timed step)")
    oracle = Oracle.from_hip_model(model)

    def step():
        losses = oracle.losses(data, *extra)
        total = sum(losses.values())
        tr = oracle.trainable()
        grads = torch.autograd.grad(total, list(tr.values()), allow_unused=True)
        oracle.sgd_step({k: (g if g is not None else torch.zeros_like(v)) for (k, v), g in zip(tr.items(), grads)}, {}, 0.01)

    t0 = time.time()
    step()
    first = time.time() - t0
    warm, steps = args.cpu_warmup, args.cpu_steps
    if first * (warm + steps) > 60.0:            # bound the leg: ~45 s, never fewer than 1 warm-up + 2 timed steps
        warm, steps = 1, max(2, min(steps, int(45.0 / first) - 1))
    for _ in range(warm - 1):
        step()
    t1 = time.time()
    for _ in range(steps):
        step()
    dt = time.time() - t1
    cpu = ""
    try:
        cpu = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except Exception:
        pass
    return {"value": round(n * steps / dt, 4), "unit": "img/s", "cores": cores, "kind": "port",
            "sample": f"{n} synthetic 1333x800 image(s) per step, {warm} warm-up + {steps} timed full training steps (fwd+bwd+SGD) of the "
                      f"fp32 CPU oracle ({Oracle.__name__}){note}, {dt:.1f} s timed ({time.time() - t0:.1f} s in all); host: {os.cpu_count()} logical CPUs, {cpu}"}


DUMP_SAMPLE = 1 << 22       # elements of the parameter arena --dump-outputs writes (16 MB in float32)


def snapshot_outputs(losses, total, arena):
    """What the last timed step hands its caller, on the host: its losses (float32 scalars, as computed) and a fixed sample of the
    parameter arena it updated (float32; the DUMP_SAMPLE indices that a generator seeded with 0 draws from the arena, in increasing order -
    the whole arena when it is smaller).  Same arguments -> same indices, so two builds compare element for element.  The gradient arena is
    left out: it is the step's scratch (zeroed by the next step), and its backbone entries depend on the order in which the float-atomic
    reductions meet - two runs of one build differ there by up to half of a tensor's largest entry (SOD_DETERMINISTIC=1 makes runs
    bit-identical, at a cost in speed)."""
    import numpy as np

    out = {k: np.asarray(float(v.detach()), dtype=np.float32) for k, v in losses.items()}
    out["total_loss"] = np.asarray(float(total.detach()), dtype=np.float32)
    p = arena.params.detach().reshape(-1)
    n = p.numel()
    if n > DUMP_SAMPLE:
        p = p[torch.from_numpy(np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))).to(p.device)]
    out["params_sample"] = p.float().cpu().numpy()
    return out


def write_outputs(out_dir, arrays):
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


class _StdoutToStderr:
    """RCCL prints a version banner on STDOUT when its first communicator comes up; the contract of this script is ONE JSON line there.
    While the process group is created (eager communicator: ``device_id``) and the first collectives run, file descriptor 1 points to
    stderr."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)


def rccl_info(log_pattern):
    """What RCCL says it built for this rank's communicator (from its INIT / GRAPH log, captured once at start-up): channel counts, how
    many rings / trees, the transports.  It picks the algorithm (ring / tree) and protocol per CALL from these and the message size;
    that choice is only visible under NCCL_DEBUG_SUBSYS=TUNING, which prints per collective and is therefore not enabled in a timed
    run.  Best effort: None when nothing was captured."""
    import glob
    import re

    if not log_pattern:
        return None
    info = {"version": None, "channels": None, "rings": 0, "trees": 0, "transports": []}
    try:
        text = ""
        for f in glob.glob(os.path.join(os.path.dirname(log_pattern), "*")):
            with open(f, errors="replace") as fh:
                text += fh.read()
        m = re.search(r"(RCCL|NCCL) version ([^\s]+)", text)
        info["version"] = m.group(2) if m else None
        m = re.search(r"(\d+) coll channels, (\d+) (?:collnet|nvls) channels.*?(\d+) p2p channels", text)
        if m:
            info["channels"] = {"coll": int(m.group(1)), "p2p": int(m.group(3))}
        info["rings"] = len(set(re.findall(r"Channel (\d+)/\d+\s*:", text)))
        info["trees"] = len(re.findall(r"Trees \[", text))
        info["transports"] = sorted(set(re.findall(r"via ([A-Za-z0-9/_]+)", text)))[:8]
        m = re.search(r"comm 0x[0-9a-f]+ rank \d+ nranks (\d+)", text)
        info["nranks"] = int(m.group(1)) if m else None
        info["log_bytes"] = len(text)
    except Exception as e:      # noqa: BLE001 - reporting only
        info["error"] = repr(e)[:120]
    return info


def device_fingerprint(index=0, clocks_only=False):
    """Which device produced the line: MI355X parts differ by several per cent at equal code (clocks under load, power cap), so a
    reader comparing two runs needs to know whether they ran on the same one.  Best effort, never fails the benchmark."""
    fp = {}
    try:
        if clocks_only:
            raise LookupError
        p = torch.cuda.get_device_properties(index)
        fp["name"] = p.name
        uuid = str(getattr(p, "uuid", "") or "")
        if uuid:
            fp["uuid_tail"] = uuid[-8:]
        fp["cus"] = p.multi_processor_count
    except Exception:
        pass
    try:
        import glob
        cards = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
        if cards:
            # the sysfs card of THIS device: a one-GPU box still lists every card of the host, so the card is matched by PCI address
            # (hipDeviceGetPCIBusId); until round 5 card<index> was read - another GPU's clock
            base, pci = None, None
            try:
                import ctypes
                # the HIP runtime torch has ALREADY loaded (its exact path from the process map: dlopen returns that handle, never a second copy)
                loaded = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l})
                if loaded:
                    hip = ctypes.CDLL(loaded[0])
                    buf = ctypes.create_string_buffer(64)
                    if hip.hipDeviceGetPCIBusId(buf, 64, int(index)) == 0:
                        pci = buf.value.decode().lower()
            except Exception:
                pci = None
            if pci:
                for c in cards:
                    if os.path.basename(os.path.realpath(os.path.dirname(c))).lower() == pci:
                        base = os.path.dirname(c)
            fp["sysfs_card"] = os.path.basename(os.path.dirname(base)) if base else "unmatched (card%d read)" % min(index, len(cards) - 1)
            if base is None:
                base = os.path.dirname(cards[min(index, len(cards) - 1)])
            levels = [l.strip() for l in open(os.path.join(base, "pp_dpm_sclk")).read().splitlines() if l.strip()]
            fp["sclk_levels"] = [l.split(":")[1].strip().rstrip("*").strip() for l in levels][-2:]
            fp["sclk_active"] = next((l.split(":")[1].strip().rstrip("*").strip() for l in levels if l.endswith("*")), None)
            caps = glob.glob(os.path.join(base, "hwmon", "hwmon*", "power1_cap"))
            if caps:
                fp["power_cap_w"] = int(open(caps[0]).read().strip()) // 1000000
            for f in ("unique_id", "serial_number"):
                q = os.path.join(base, f)
                if os.path.exists(q) and "uuid_tail" not in fp:
                    fp["uuid_tail"] = open(q).read().strip()[-8:]
    except Exception:
        pass
    return fp


def launcher_cmd(nproc):
    """``torch.distributed.run`` for ``nproc`` ranks of this node.  No port is guessed here: the agent's c10d rendezvous binds port 0
    itself (the kernel picks a free one while the socket stays open) and the ranks reuse that store - binding a probe socket, closing
    it and handing the number on is a race (EADDRINUSE when anything else takes the port in between)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--rdzv-backend", "c10d",
            "--rdzv-endpoint", "127.0.0.1:0", "--local-addr", "127.0.0.1"]


def spawn_ranks(args, argv):
    """``python bench.py --gpus N`` (N > 1, no launcher around it): start the N ranks ourselves, one process per GPU, as the
    reference's train_net.py does through detectron2's ``launch`` (/root/reference/train_net.py:185-195).  This process has not
    touched the GPU yet (``torch.cuda.device_count()`` does not initialise it on this image) and never will: the ranks are fresh
    children of ``torch.distributed.run``; rank 0 prints the JSON line, which is relayed unchanged."""
    import subprocess

    share = os.environ.get("SOD_BENCH_SHARE_GPU") == "1"
    have = torch.cuda.device_count()
    if not share and have < args.gpus:
        print(f"bench.py: --gpus {args.gpus} requested but this node exposes {have} GPU(s)", file=sys.stderr)
        sys.exit(2)
    cmd = launcher_cmd(args.gpus) + [os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rc = subprocess.call(cmd, env=env)
    sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch-per-gpu", type=int, default=16)
    ap.add_argument("--cpu-images", type=int, default=2)
    ap.add_argument("--cpu-warmup", type=int, default=3)
    ap.add_argument("--cpu-steps", type=int, default=10)
    ap.add_argument("--cpu-threads", type=int, default=32)
    ap.add_argument("--depth", type=int, default=50, help="ResNet depth (tests use 18; the benchmark is R50)")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--arch", choices=sorted(ARCH_NAMES), default="fcos", help="fcos = the headline metric (BASELINE.json configs[1])")
    ap.add_argument("--resnext", action="store_true", help="ResNeXt 32x8d bottlenecks (configs/ablation_studies/*/base_X101.yaml: NUM_GROUPS 32, "
                    "WIDTH_PER_GROUP 8, STRIDE_IN_1X1 False) instead of ResNet: the grouped-convolution path; not the headline")
    ap.add_argument("--base-lr", type=float, default=None, help="override SOLVER.BASE_LR (experiments: e.g. RepPoints at the reference's 0.01, where "
                    "random initialisation diverges and the learned offsets grow)")
    ap.add_argument("--reppoints-offset-px", type=float, default=0.0, help="experiment (reppoints): the biases of the initial point "
                    "prediction drawn from N(0, S px), i.e. DeformConv offsets S pixels (of the level) away from the kernel grid as a trained "
                    "detector's are - how far the step time depends on the offsets leaving the backward kernel's LDS window")
    ap.add_argument("--constant-lr", action="store_true", help="constant SOLVER.BASE_LR from step 0 instead of the reference's WarmupMultiStepLR")
    ap.add_argument("--bucket-mb", type=float, default=None, help="N > 1: size of the gradient all-reduce buckets (default 32 MB)")
    ap.add_argument("--wire", choices=["fp32", "bf16"], default=None, help="N > 1: wire format of the gradient buckets (default fp32, SOD_GRAD_BUCKET_DTYPE)")
    ap.add_argument("--collective", choices=["all_reduce", "rs_ag"], default=None, help="N > 1: shape of the gradient exchange per bucket - one all-reduce "
                    "(default) or reduce-scatter + all-gather (SURVEY.md 8 e; SOD_GRAD_COLLECTIVE)")
    ap.add_argument("--no-rccl-info", action="store_true", help="N > 1 / rehearsal: do not capture RCCL's INIT log (channels, rings / trees) into config.rccl_info")
    ap.add_argument("--full", action="store_true", help="beside the headline: the roofline of sampled timed steps, the CPU oracle baseline, "
                    "the host probes and the device fingerprint (each can be left out with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step hands its caller to DIR/<name>.npy: "
                    "its losses and a fixed, seeded sample of the parameters it updated (snapshot_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no cpu_baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: no roofline (no sampled steps)")
    ap.add_argument("--dump-prof", type=int, default=0, help="with --full: print the N most expensive (kernel, shape) groups to stderr")
    ap.add_argument("--rccl-rehearsal", action="store_true",
                    help="--gpus 1 only: create a one-rank RCCL process group and issue every data-parallel collective anyway (parameter "
                         "broadcast, normaliser all-reduce, bucketed gradient all-reduce) - exercises the real RCCL path on a one-GPU box")
    ap.add_argument("--hw-queues", type=int, default=0, help="GPU_MAX_HW_QUEUES for this run (default: the runtime's 4 on one GPU, 6 for "
                    "data-parallel ranks and the rehearsal - utils/comm.py:prepare_rank_env)")
    ap.add_argument("--no-host-probe", action="store_true", help="with --full: skip the three un-timed steps after the loop that measure the host's "
                    "enqueue time into empty queues (a plain run never takes them: its trace holds exactly warm-up + timed steps)")
    ap.add_argument("--sync-debug", action="store_true", help="diagnostic: torch.cuda.set_sync_debug_mode('warn') during the timed loop - every "
                    "call site that makes the host wait for the device prints a warning with its stack (the step must have none)")
    ap.add_argument("--rehearsal-occupancy", default=None, metavar="WGS:GBPS",
                    help="with --rccl-rehearsal: every bucket's all-reduce is followed on the communication stream by WGS resident workgroups for "
                         "the time an 8-rank ring takes at GBPS of bus bandwidth (sod_debug_occupy) - what the step loses while RCCL's channel "
                         "kernels hold CUs; e.g. 32:300")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    # what a plain run leaves out: everything beside the headline figure
    args.no_roofline = args.no_roofline or not args.full
    args.no_cpu_baseline = args.no_cpu_baseline or not args.full
    args.no_host_probe = args.no_host_probe or not args.full

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args, sys.argv[1:])         # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} does not match the launcher's WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.hw_queues:
        os.environ["GPU_MAX_HW_QUEUES"] = str(args.hw_queues)
    from slenderobjdet_amd.utils import comm as _comm_mod
    _comm_mod.prepare_rank_env(world, rehearsal=args.rccl_rehearsal)      # nothing has touched the GPU yet: the HIP runtime reads these at start-up
    rccl_log = None
    if (world > 1 or args.rccl_rehearsal) and not args.no_rccl_info and "NCCL_DEBUG" not in os.environ and os.environ.get("SOD_BENCH_SHARE_GPU") != "1":
        # RCCL's own account of what it built (channel count, rings / trees, transport): INIT-time lines only, into a file per rank -
        # nothing is printed per collective call, so the timed loop is unaffected
        import tempfile
        rccl_log = os.path.join(tempfile.mkdtemp(prefix="sod_rccl_"), "rccl.%h.%p.log")
        os.environ.update(NCCL_DEBUG="INFO", NCCL_DEBUG_SUBSYS="INIT,GRAPH,ENV", NCCL_DEBUG_FILE=rccl_log)
    if world > 1:
        # SOD_BENCH_SHARE_GPU=1 (tests only): every rank uses cuda:0 with the gloo backend, to exercise the data-parallel
        # path on a single-GPU box; the real launch is one rank per GPU over RCCL ("nccl").
        share = os.environ.get("SOD_BENCH_SHARE_GPU") == "1"
        dev_index = 0 if share else local_rank
        torch.cuda.set_device(dev_index)
        if share:
            dist.init_process_group("gloo")
        else:
            with _StdoutToStderr():
                dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
                dist.barrier()
    else:
        torch.cuda.set_device(0)
        if args.rccl_rehearsal:
            with _StdoutToStderr():     # a one-rank group needs no TCP rendezvous: an in-process store
                dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
                dist.barrier()
    dev = torch.device("cuda", torch.cuda.current_device())
    rehearsal = args.rccl_rehearsal and world == 1
    if rehearsal:
        from slenderobjdet_amd.utils import comm as _comm
        _comm.FORCE_COLLECTIVES = True

    from slenderobjdet_amd import _C
    from slenderobjdet_amd.data import SyntheticCocoBatches
    from slenderobjdet_amd.layers import functional as HF
    from slenderobjdet_amd.modeling import build_model
    from slenderobjdet_amd.solver import build_optimizer

    cfg = make_cfg(args.depth, args.arch, constant_lr=args.constant_lr)
    if args.base_lr is not None:
        cfg.SOLVER.BASE_LR = args.base_lr
    if args.resnext:
        cfg.MODEL.RESNETS.NUM_GROUPS, cfg.MODEL.RESNETS.WIDTH_PER_GROUP, cfg.MODEL.RESNETS.STRIDE_IN_1X1 = 32, 8, False
    torch.manual_seed(1 + rank)   # engine/defaults.py:66: SEED + rank
    model = build_model(cfg)
    model.train()
    if args.arch in ("retinanet", "rrcnn") and args.depth >= 50:
        damp_residual_branches(model)
    if args.reppoints_offset_px > 0:
        assert args.arch == "reppoints", "--reppoints-offset-px needs --arch reppoints"
        with torch.no_grad():
            b = model.offsets_init[1].conv.bias
            b[: 2 * model.num_points].copy_(torch.randn(2 * model.num_points, generator=torch.Generator().manual_seed(5)) * args.reppoints_offset_px)
        model.arena.bump()
    if args.bucket_mb is not None or args.wire is not None or args.collective is not None:
        model.arena.configure_buckets(args.bucket_mb if args.bucket_mb is not None else 32.0, args.wire, args.collective)
    if args.rehearsal_occupancy:
        assert rehearsal, "--rehearsal-occupancy needs --rccl-rehearsal on one GPU"
        wgs, gbps = args.rehearsal_occupancy.split(":")
        model.arena.rehearsal_occupancy = (int(wgs), float(gbps), 8)
    if world > 1 or rehearsal:   # DDP semantics: identical initial parameters on every rank
        dist.broadcast(model.arena.params, src=0)
        model.arena.bump()
    optimizer = build_optimizer(cfg, model)
    optimizer.grad_scale = 1.0 / world
    # The reference's schedule (configs/fcos/Base-Fcos.yaml:14-18 -> detectron2 WarmupMultiStepLR: linear warm-up from 1e-3 x BASE_LR over
    # the first 1000 iterations), stepped once per iteration as DefaultTrainer does; --constant-lr = a constant BASE_LR from step 0 (rounds 1-4)
    scheduler = None
    if not args.constant_lr:
        from slenderobjdet_amd.solver import build_lr_scheduler
        scheduler = build_lr_scheduler(cfg, optimizer)
    loader = SyntheticCocoBatches(args.batch_per_gpu, args.height, args.width, rank=rank, device=dev, pool=2, rotated=args.arch == "rrcnn")

    if os.environ.get("SOD_CUMASK_MAIN"):          # experiment: the whole step on a stream confined to a subset of the CUs (layers/functional.make_stream)
        _main = HF.make_stream(dev, 0, "MAIN")
        _main.wait_stream(torch.cuda.current_stream())
        torch.cuda.set_stream(_main)
    sample_at = set() if args.no_roofline else (set(range(args.steps)) if args.dump_prof else set(range(args.steps // 2, args.steps, 32)))
    sample_at = set(sorted(sample_at)[:12])      # the library keeps 8192 event pairs
    cur = next(loader)
    for w in range(args.warmup):
        nxt = next(loader)
        train_step(model, optimizer, cur, None if (w == args.warmup - 1 and 0 in sample_at) else nxt, scheduler)
        cur = nxt
    if world > 1 or rehearsal:
        dist.barrier()
    torch.cuda.synchronize()
    if not args.no_roofline:
        # The library records one hipEvent pair on the LAUNCH stream around the main kernel of every conv dispatch (forward, data
        # gradient, weight gradient: sod_conv_prof_enable) of the sampled steps.  In a normal step the data-gradient chain (main
        # stream) and the weight gradients (side stream, layers/functional.py) share the GPU, and the interval of a backward kernel
        # would then include the time it shares the chip with another kernel.  The SAMPLED steps therefore launch the weight
        # gradients on the main stream (what SOD_WGRAD_STREAM=0 does for a whole run; profiles/*_serial_kernel_stats.csv is the
        # rocprofv3 summary of such a run): intervals are per-kernel durations.  A sampled step is ~5 % slower and carries a few us
        # of queue bubbles per event pair, so only one timed step in 32 is sampled, starting in the middle of the run (all steps with --dump-prof); `value` includes them.
        HF.PROFILE_KINDS = None
        HF.PROFILE_LIB = True
    prof_all, prof_steps = [], 0
    if world > 1 or rehearsal:
        model.arena.comm_probe = []
    side_default = HF.WGRAD_SIDE_STREAM
    from slenderobjdet_amd.modeling.meta_arch import fcos as fcos_mod
    tower_default = fcos_mod.TOWER_STREAMS
    sclk_mid = None
    if args.sync_debug:
        import warnings
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
    # how far the host runs AHEAD of the device: a device event + a host time stamp at the start of every timed step (a profiler slows the
    # host down, so only the un-profiled run can say); lead_i = (device time of event i) - (host time of its record call)
    lead_ev, lead_host = [], []
    torch.cuda.synchronize()
    if args.full:
        base_ev = torch.cuda.Event(enable_timing=True)
        base_ev.record()
        torch.cuda.synchronize()
        base_host = time.perf_counter()
    last_losses = {} if args.dump_outputs else None
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.full:
            ev_i = torch.cuda.Event(enable_timing=True)
            lead_host.append(time.perf_counter())
            ev_i.record()
            lead_ev.append(ev_i)
        if args.full and i == (3 * args.steps) // 4 and rank == 0:
            # the shader clock the device reports WHILE the timed loop keeps it busy (a sysfs read: no GPU call, ~50 us of host time; the
            # host runs several steps ahead of the device); read after the loop it is the idle clock
            sclk_mid = device_fingerprint(dev.index or 0, clocks_only=True).get("sclk_active")
        sample = i in sample_at       # one timed step in 32, the first in the middle of the run (all of them with --dump-prof)
        HF.PROFILE = prof_all if sample else None
        if HF.PROFILE_LIB:
            _C.call("sod_conv_prof_enable", 1 if sample else 0)
        prof_steps += int(sample)
        HF.WGRAD_SIDE_STREAM = side_default and not sample
        fcos_mod.TOWER_STREAMS = tower_default and not sample
        # a sampled step computes its own frozen prefix on the main stream (so that its profile holds every conv of a step) and hands
        # none to its successor
        nxt = next(loader)
        last = train_step(model, optimizer, cur, None if (sample or (i + 1) in sample_at) else nxt, scheduler,
                          last_losses if i == args.steps - 1 else None)
        cur = nxt
    HF.WGRAD_SIDE_STREAM = side_default
    fcos_mod.TOWER_STREAMS = tower_default
    host_dt = time.perf_counter() - t0          # the host has ENQUEUED the K steps; the device is still working on them
    if args.sync_debug:
        torch.cuda.set_sync_debug_mode("default")
    if world > 1 or rehearsal:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof, HF.PROFILE = prof_all, None
    # the last timed step's results, before anything else (the host probe's steps) runs on the model
    outputs = snapshot_outputs(last_losses, last, model.arena) if args.dump_outputs and rank == 0 else None
    leads = sorted(base_ev.elapsed_time(e) * 1e-3 - (h - base_host) for e, h in zip(lead_ev[2:], lead_host[2:])) if args.full else []
    host_lead_ms = (round(leads[0] * 1e3, 2), round(leads[len(leads) // 2] * 1e3, 2)) if leads else None
    # Host time of ONE step with empty queues (outside the timed region): how long Python + the launch path need to enqueue a step when
    # nothing blocks them.  host_enqueue_ms_per_step above converges to the device's step time once the launch queues are full, so it cannot
    # tell whether the host is the limiter; this one can (host-bound if it approaches ms_per_step).
    host_unblocked = []
    for _ in range(0 if args.no_host_probe else 3):
        nxt = next(loader)
        torch.cuda.synchronize()
        th = time.perf_counter()
        last = train_step(model, optimizer, cur, nxt, scheduler)
        host_unblocked.append(time.perf_counter() - th)
        cur = nxt
    torch.cuda.synchronize()
    if HF.PROFILE_LIB:
        import ctypes
        _C.call("sod_conv_prof_enable", 0)
        lib_entries = [p_ for p_ in prof if p_[2] is None]      # entries timed by the library; the rest carry their own torch events
        n = len(lib_entries)
        ms, var, frac, mode = (ctypes.c_float * max(n, 1))(), (ctypes.c_int * max(n, 1))(), (ctypes.c_float * max(n, 1))(), (ctypes.c_int * max(n, 1))()
        got = _C.load().sod_conv_prof_collect(ms, var, frac, mode, n)
        kinds = {"conv_fwd": 0, "conv_dgrad": 1, "conv_wgrad": 2}
        if got != n or any(kinds[p_[0]] != mode[j] for j, p_ in enumerate(lib_entries)):
            # never fail the measurement over the instrumentation: drop the roofline instead
            print(f"# roofline skipped: library recorded {got} conv dispatches, host {n} (or their order differs)", file=sys.stderr)
            prof = []
        else:
            filled, j = [], 0
            for kind, flops, e0, e1, desc, variant in prof:
                if e0 is None:
                    filled.append((kind, flops * frac[j], ms[j] * 1e-3, desc, var[j]))
                    j += 1
                else:
                    filled.append((kind, flops, e0.elapsed_time(e1) * 1e-3, desc, variant))
            prof = filled
        HF.PROFILE_LIB = False
    if world > 1 or rehearsal:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    dump = os.environ.get("SOD_BENCH_DUMP_PARAMS")
    if dump:   # tests: replicas must stay bit-identical
        torch.save(model.arena.params.detach().cpu(), os.path.join(dump, f"params_rank{rank}.pt"))
    loss_val = float(last.detach())
    # A step that silently produced garbage must not print a number: the last step's loss has to be finite and in the band a detector
    # loss lives in, and the gradient arena it left behind finite and non-zero (every trainable tensor is written by the backward pass).
    gnorm = float(model.arena.grads.float().norm())
    if not (loss_val == loss_val and abs(loss_val) < 1e4):
        print(f"bench.py: final loss {loss_val} is not a sane training loss", file=sys.stderr)
        sys.exit(3)
    if not (gnorm == gnorm and 0.0 < gnorm < 1e12):
        print(f"bench.py: gradient norm {gnorm} after the last step (NaN / zero / overflow)", file=sys.stderr)
        sys.exit(3)

    if rank == 0:
        imgs = args.steps * args.batch_per_gpu * world
        out = {
            "metric": f"training img/sec {ARCH_NAMES[args.arch]} R{args.depth}-FPN 1333x800", "value": round(imgs / dt, 3), "unit": "img/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": WORKLOADS[args.arch] + (" [ResNeXt 32x8d backbone]" if args.resnext else ""), "global_batch": args.batch_per_gpu * world, "parallelism": f"dp{world}",
                       "final_loss": round(loss_val, 5), "final_grad_norm": round(gnorm, 5), "base_lr": cfg.SOLVER.BASE_LR,
                       **({"reppoints_offset_px": args.reppoints_offset_px} if args.reppoints_offset_px > 0 else {}),
                       "lr_schedule": ("constant" if scheduler is None else
                                       f"{cfg.SOLVER.LR_SCHEDULER_NAME}: {cfg.SOLVER.WARMUP_METHOD} warm-up from {cfg.SOLVER.WARMUP_FACTOR} x base over "
                                       f"{cfg.SOLVER.WARMUP_ITERS} iterations, stepped every iteration (lr at the last step {optimizer.param_groups[0]['lr']:.3e})"),
                       "host_enqueue_ms_per_step": round(host_dt / args.steps * 1e3, 3),
                       "host_ms_per_step_unblocked": round(min(host_unblocked) * 1e3, 3) if host_unblocked else None,
                       "host_lead_ms_min_median": host_lead_ms},     # device start of a step minus the host's enqueue time of that start
        }
        if args.full:
            out["config"]["device"] = device_fingerprint(dev.index or 0)
            out["config"]["device"]["sclk_active"] = sclk_mid      # sampled at 3/4 of the timed loop (None if sysfs does not expose it)
        ref_lr = {"fcos": 0.01, "retinanet": 0.01, "reppoints": 0.01, "rrcnn": 0.02}[args.arch]
        if cfg.SOLVER.BASE_LR != ref_lr:        # not the reference configuration's rate: say so in the line (round-3 advisor finding)
            out["config"]["base_lr_note"] = (f"reference config trains at {ref_lr} from an ImageNet checkpoint; random initialisation diverges there "
                                             "(DESIGN.md section 4), and for reppoints the diverging offsets leave the DeformConv kernels' LDS windows")
        if world > 1 or rehearsal:
            # what the collective layer saw, so that a reader of this line can check that the run was the N-rank data-parallel job it
            # claims (reference: train_net.py:185-195 -> detectron2 launch -> one process per GPU, NCCL all-reduce of every gradient)
            ar = model.arena
            pairs = (getattr(ar, "comm_probe", None) or [])[:args.steps]      # (the three un-timed host-latency steps after the loop excluded)
            exposed = [a.elapsed_time(b) for a, b in pairs]
            out["config"].update({
                "backend": dist.get_backend(), "ranks_seen": dist.get_world_size(), "bucket_mb": round(ar.bucket_elems * 4 / (1 << 20), 1),
                "n_buckets": len(ar.buckets), "bucket_mb_each": [round((e - b) * 4 / (1 << 20), 1) for b, e in ar.buckets], "grad_bytes_per_step": int(ar.total * (4 if ar.bucket_dtype == torch.float32 else 2)),
                "wire_dtype": str(ar.bucket_dtype).replace("torch.", ""), "collective": ar.collective,
                "rccl_info": rccl_info(rccl_log),
                "exposed_comm_ms_per_step": round(sum(exposed) / len(exposed), 3) if exposed else None,
                "exposed_comm_note": "rank 0, mean over the timed steps: compute-stream idle time between the end of backward and the end of the last bucket's all-reduce",
                # what RCCL was told (it picks ring / tree and the channel count per call itself; NCCL_DEBUG=INFO prints its choices to stderr)
                "rccl_env": {k: os.environ[k] for k in sorted(os.environ) if k.startswith(("NCCL_", "RCCL_"))},
                "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default (4)"),
                # set in-process after the HIP runtime had started (e.g. under rocprofv3): requested, not what the runtime used
                "hw_queues_effective": not _comm_mod.HIP_STARTED_BEFORE_PREPARE})
        if rehearsal:
            out["config"]["rccl_rehearsal"] = "one-rank RCCL group, every data-parallel collective issued"
            if args.rehearsal_occupancy:
                out["config"]["rehearsal_occupancy"] = args.rehearsal_occupancy + " (WGS:GBPS, emulated 8-rank ring occupancy per bucket)"
        if args.arch == "fcos" and args.depth == 50:
            # SURVEY.md 8(d)'s 1.1913 TFLOP per image is an UPPER bound (it counts a data gradient for the first trainable layer);
            # roofline.by_pass sums the FLOPs of the launches actually timed
            out["model_tflops_upper_bound"] = round(imgs * TRAIN_FLOP_PER_IMAGE / dt / 1e12, 2)
        if prof:
            out["roofline"] = roofline_report(prof, prof_steps, args)
            if prof_steps:
                out["timed_conv_tflop_per_step"] = round(sum(p_[1] for p_ in prof) / prof_steps / 1e12, 3)
        if prof and args.dump_prof:
            per = {}
            for kind, flops, sec_, desc, _variant in prof:
                a = per.setdefault((kind, desc), [0.0, 0.0, 0])
                a[0] += flops; a[1] += sec_; a[2] += 1
            for (kind, desc), (fl, sec, cnt) in sorted(per.items(), key=lambda kv: -kv[1][1])[:args.dump_prof]:
                print(f"# {kind:10s} NHWCKRs={desc} calls/step {cnt // prof_steps:3d} ms/step {sec / prof_steps * 1e3:7.3f} TF/s {fl / sec / 1e12:7.1f}", file=sys.stderr)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(model, args)
        if outputs is not None:
            write_outputs(args.dump_outputs, outputs)
        print(json.dumps(out), flush=True)
    if world > 1 or rehearsal:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
