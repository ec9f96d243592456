#!/usr/bin/env python
"""Golden vectors for the RetinaNet and the RPN / proposal half of the two-stage path, produced by the REFERENCE's own Python
(read-only /root/reference) in the build container.  Only inputs / outputs (numpy arrays) and meta.json are written; no reference
source is copied.

The four reference files are loaded with importlib under stub modules and their methods run unbound on a SimpleNamespace ``self``:

  retina/retina_rotated.py          permute_to_N_HWA_K :25-34, losses :185-249, label_anchors :251-295, inference_single_image :319-378
  proposal_generator/rpn.py         label_and_sample_anchors :136-191, losses :193-251, the reshapes of forward :278-289,
                                    _decode_proposals :337-356
  proposal_generator/proposal_utils.py   find_top_rpn_proposals_anchors :11-130
  roi_heads/fast_rcnn.py            fast_rcnn_inference_single_image_with_anchor :53-115

RESTATED third-party parts (detectron2 / fvcore exist nowhere): Matcher, Box2BoxTransform(Rotated), pairwise_iou for 4- and
5-column boxes, batched_nms, smooth_l1_loss, giou_loss, sigmoid focal loss, Boxes.clip / nonempty are oracle/'s restatements
(oracle/detection.py, oracle/rcnn.py, oracle/losses.py); ``Boxes`` / ``Instances`` below are containers; get_event_storage().put_scalar
does nothing, retry_if_cuda_oom is the identity, subsample_labels records what it is handed and returns a fixed seeded subset.
retina_rotated.py:375 names ``Boxes`` without importing it: the container below is put into the module's namespace.

Every float-valued function runs twice, in fp32 (the fixture value ``x``) and on float64 inputs (``x_f64``); the spread between the
two is the yardstick of the tests' tolerances.  Before anything is written the generator asserts, in float64, that no decision of a
fixture hangs on float rounding (margins below) and that every edge case a fixture is meant to hold is exercised.

    python tests/golden/retina_rpn/make_golden_retina_rpn.py
"""
import importlib.util
import io
import json
import math
import os
import sys
import types
import zipfile
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(OUT, "..", "..", ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import detection as od      # noqa: E402
from oracle import losses as ol         # noqa: E402
from oracle import rcnn as orc          # noqa: E402
import rotated_iou_loss_restated as rr  # noqa: E402  (float64 rotated IoU by polygon clipping)

F32, F64 = torch.float32, torch.float64
HW = [(8, 10), (4, 5), (2, 3)]
STRIDES = [8, 16, 32]
A, K, N = 3, 5, 2
IMAGE_SIZES = [(64, 80), (60, 76)]
W4, W5 = (1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0, 1.0)
RPN_W4, RPN_W5 = (1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0, 1.0)
MARGIN = {4: 1e-5, 5: 4e-4}       # distance of every deciding IoU from a threshold (5: twice the suite's 2e-4 bar on box_iou_rotated)
SCALE_CLAMP = math.log(1000.0 / 16)
NMS_LOG = []                       # one entry per batched_nms call: candidates, survivors


# ------------------------------------------------------------------------------------------------ containers and restated parts
class Boxes:
    """Container for (n, 4) XYXY or (n, 5) (cx, cy, w, h, angle) boxes: what the reference reads of detectron2's Boxes / RotatedBoxes."""

    def __init__(self, t):
        self.tensor = t

    device = property(lambda self: self.tensor.device)

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, i):
        return Boxes(self.tensor[i].view(-1, self.tensor.shape[-1]))

    def to(self, *a, **k):
        return self

    @classmethod
    def cat(cls, bl):
        return cls(torch.cat([b.tensor for b in bl]))

    def clip(self, size):          # RESTATED Boxes.clip / RotatedBoxes.clip (oracle/rcnn.py)
        self.tensor = orc.clip_boxes(self.tensor, size)

    def nonempty(self, threshold=0.0):      # RESTATED (oracle/rcnn.py)
        return orc.nonempty(self.tensor, threshold)


class Instances:
    def __init__(self, image_size):
        object.__setattr__(self, "_f", {})
        object.__setattr__(self, "image_size", image_size)

    def __setattr__(self, k, v):
        self._f[k] = v

    def __getattr__(self, k):
        try:
            return object.__getattribute__(self, "_f")[k]
        except KeyError:
            raise AttributeError(k)

    def get_fields(self):
        return self._f


class GT(NS):
    def __len__(self):
        return len(self.gt_boxes)


def iou_matrix(t1, t2):
    """RESTATED pairwise_iou: 4 columns in the inputs' dtype; 5 columns oracle.detection's fp32 emulation of box_iou_rotated, or
    float64 polygon clipping for float64 inputs."""
    if len(t1) == 0:
        return torch.zeros((0, len(t2)), dtype=t2.dtype)
    if t1.shape[1] == 4:
        a1 = (t1[:, 2] - t1[:, 0]) * (t1[:, 3] - t1[:, 1])
        a2 = (t2[:, 2] - t2[:, 0]) * (t2[:, 3] - t2[:, 1])
        wh = (torch.min(t1[:, None, 2:], t2[:, 2:]) - torch.max(t1[:, None, :2], t2[:, :2])).clamp(min=0)
        inter = wh.prod(dim=2)
        return torch.where(inter > 0, inter / (a1[:, None] + a2 - inter), torch.zeros(1, dtype=inter.dtype))
    if t1.dtype == F64:
        G, R = len(t1), len(t2)
        return rr.iou(t1[:, None].expand(G, R, 5).reshape(-1, 5), t2[None].expand(G, R, 5).reshape(-1, 5)).view(G, R)
    return od.pairwise_iou_rotated(t1, t2)


def pairwise_iou(b1, b2):
    return iou_matrix(b1.tensor, b2.tensor)


class Matcher:
    """RESTATED detectron2 Matcher (oracle/detection.py)."""

    def __init__(self, thresholds, labels, allow_low_quality_matches=False):
        self.thresholds, self.labels, self.allow = list(thresholds), list(labels), allow_low_quality_matches

    def __call__(self, q):
        return od.matcher(q, self.thresholds, self.labels, self.allow)


class B2B:
    """RESTATED Box2BoxTransform / Box2BoxTransformRotated (oracle/rcnn.py, both branches)."""

    def __init__(self, weights):
        self.weights = weights

    def get_deltas(self, src, tgt):
        return orc.get_deltas(src, tgt, self.weights)

    def apply_deltas(self, deltas, boxes):
        if len(deltas) == 0:
            return deltas.new_zeros((0, deltas.shape[1]))
        return orc.apply_deltas(deltas, boxes, self.weights)


def _greedy(iou, scores, groups, thr):
    order = torch.sort(scores, descending=True, stable=True).indices.tolist()
    dead, keep = set(), []
    for p, i in enumerate(order):
        if i in dead:
            continue
        keep.append(i)
        for j in order[p + 1:]:
            if groups[j] == groups[i] and iou[i, j] > thr:
                dead.add(j)
    return torch.tensor(keep, dtype=torch.int64)


def batched_nms(boxes, scores, idxs, thr):
    """RESTATED batched_nms (oracle/rcnn.py batched_nms_any on the fp32 values: the fixture's result), checked against a per-group greedy
    NMS on float64 IoUs; asserts the NMS margins and the distinct scores on the way."""
    D = boxes.shape[1]
    s32 = scores.float()
    assert torch.unique(s32).numel() == s32.numel(), "scores entering NMS must be pairwise distinct in fp32"
    keep = orc.batched_nms_any(boxes.float(), s32, idxs, thr)
    M, b64 = len(boxes), boxes.double()
    same = (idxs[:, None] == idxs[None]) & ~torch.eye(M, dtype=torch.bool)
    q = torch.zeros((M, M), dtype=F64)
    pi, pj = torch.nonzero(torch.triu(same), as_tuple=True)          # only pairs that can suppress each other (never a box with itself)
    if len(pi):
        if D == 5:
            v = rr.iou(b64[pi], b64[pj])
        else:
            b1, b2 = b64[pi], b64[pj]
            inter = (torch.min(b1[:, 2:], b2[:, 2:]) - torch.max(b1[:, :2], b2[:, :2])).clamp(min=0).prod(1)
            v = inter / ((b1[:, 2:] - b1[:, :2]).prod(1) + (b2[:, 2:] - b2[:, :2]).prod(1) - inter)
        q[pi, pj], q[pj, pi] = v, v
    if same.any():
        gap = (q[same] - thr).abs().min().item()
        assert gap >= MARGIN[D], f"NMS pair within {gap:.2e} of the threshold"
    keep64 = _greedy(q, scores.double(), idxs.tolist(), thr)
    assert torch.equal(keep, keep64), "fp32 offset-trick NMS and float64 per-group NMS disagree"
    NMS_LOG.append((len(boxes), len(keep)))
    return keep


class _Storage:
    def put_scalar(self, *a, **k):
        pass


class _Reg:
    def register(self, obj=None):
        return (lambda f: f) if obj is None else obj


SAMPLER = NS(seen=[], gen=None)


def subsample_labels(label, num_samples, positive_fraction, bg_label):
    """Sampling stub: records the matcher's label vector, returns a seeded subset with detectron2's counts."""
    SAMPLER.seen.append(label.clone())
    pos = torch.nonzero((label != -1) & (label != bg_label))[:, 0]
    neg = torch.nonzero(label == bg_label)[:, 0]
    npos = min(pos.numel(), int(num_samples * positive_fraction))
    nneg = min(neg.numel(), num_samples - npos)
    return pos[torch.randperm(pos.numel(), generator=SAMPLER.gen)[:npos]], neg[torch.randperm(neg.numel(), generator=SAMPLER.gen)[:nneg]]


def _stub(name, **attrs):
    m = sys.modules.get(name) or types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    m.__path__ = []
    sys.modules[name] = m
    return m


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def install():
    focal = lambda x, t, alpha=-1, gamma=2, reduction="none": ol.sigmoid_focal_loss(x, t, alpha, gamma, reduction)
    sl1 = lambda x, t, beta, reduction="none": ol.smooth_l1_loss(x, t, beta, reduction)
    giou = lambda a, b, reduction="none": ol.giou_loss_xyxy(a, b, reduction)
    _stub("fvcore")
    _stub("fvcore.nn", giou_loss=giou, sigmoid_focal_loss_jit=focal, smooth_l1_loss=sl1)
    _stub("detectron2")
    _stub("detectron2.data")
    _stub("detectron2.data.detection_utils", convert_image_to_rgb=None)
    _stub("detectron2.layers", ShapeSpec=NS, batched_nms=batched_nms, cat=torch.cat, get_norm=None, Linear=None,
          nonzero_tuple=lambda x: x.nonzero(as_tuple=True))
    _stub("detectron2.modeling")
    _stub("detectron2.modeling.anchor_generator", build_anchor_generator=None)
    _stub("detectron2.modeling.backbone", build_backbone=None)
    _stub("detectron2.modeling.box_regression", Box2BoxTransformRotated=B2B, Box2BoxTransform=B2B)
    _stub("detectron2.modeling.matcher", Matcher=Matcher)
    _stub("detectron2.modeling.meta_arch")
    _stub("detectron2.modeling.meta_arch.build", META_ARCH_REGISTRY=_Reg())
    _stub("detectron2.modeling.postprocessing", detector_postprocess=None)
    _stub("detectron2.structures", ImageList=None, Instances=Instances, RotatedBoxes=Boxes, Boxes=Boxes, pairwise_iou=pairwise_iou)
    _stub("detectron2.utils")
    _stub("detectron2.utils.events", get_event_storage=lambda: _Storage())
    _stub("detectron2.utils.memory", retry_if_cuda_oom=lambda f: f)
    _stub("detectron2.utils.registry", Registry=None)
    _stub("detectron2.config", configurable=lambda f: f)
    _stub("detectron2.modeling.sampling", subsample_labels=subsample_labels)
    _stub("detectron2.modeling.proposal_generator", build_rpn_head=None)
    _stub("detectron2.modeling.proposal_generator.proposal_utils", find_top_rpn_proposals=None)
    _stub("detectron2.modeling.proposal_generator.build", PROPOSAL_GENERATOR_REGISTRY=_Reg())
    _stub("detectron2.modeling.roi_heads")
    _stub("detectron2.modeling.roi_heads.fast_rcnn", FastRCNNOutputLayers=object)
    retina = _load("ref_retina", "slender_det/modeling/meta_arch/retina/retina_rotated.py")
    retina.Boxes = Boxes           # :375 uses the name without importing it
    putils = _load("ref_putils", "slender_det/modeling/proposal_generator/proposal_utils.py")
    frcnn = _load("ref_frcnn", "slender_det/modeling/roi_heads/fast_rcnn.py")
    _stub("refpg")
    _stub("refpg.matchers", build_matcher=None)
    _stub("refpg.proposal_generator")
    rpn = _load("refpg.proposal_generator.rpn", "slender_det/modeling/proposal_generator/rpn.py")
    # rpn.py:244 hard-codes a float32 BCE target; the float64 run needs the target in the logits' dtype (no change in fp32)
    rpn.F = NS(binary_cross_entropy_with_logits=lambda x, t, reduction="mean": F.binary_cross_entropy_with_logits(x, t.to(x.dtype), reduction=reduction))
    return retina, rpn, putils, frcnn


# ------------------------------------------------------------------------------------------------ inputs
def anchors_for(D):
    if D == 4:
        return orc.anchors(HW, STRIDES, [[16], [32], [64]], [[0.5, 1.0, 2.0]])
    return orc.anchors(HW, STRIDES, [[16], [32], [64]], [[0.5]], angles=[[-45, 0, 45]])


def _rand_box(g, D, size):
    H, W = size
    u = lambda: float(torch.rand((), generator=g))
    cx, cy = 6 + u() * (W - 12), 6 + u() * (H - 12)
    w, h = 2.0 ** (2 + 3.5 * u()), 2.0 ** (2 + 3.5 * u())
    if D == 5:
        return torch.tensor([cx, cy, w, h, u() * 180 - 90], dtype=F32)
    return torch.tensor([max(cx - w / 2, 0.0), max(cy - h / 2, 0.0), min(cx + w / 2, float(W)), min(cy + h / 2, float(H))], dtype=F32)


def _near_anchor(g, anc, D):
    u = lambda: float(torch.rand((), generator=g))
    a = anc[int(torch.randint(0, 240 + 60, (), generator=g))].clone()
    if D == 4:
        w, h = a[2] - a[0], a[3] - a[1]
        cx, cy = (a[0] + a[2]) / 2 + (u() - 0.5) * 0.16 * w, (a[1] + a[3]) / 2 + (u() - 0.5) * 0.16 * h
        w, h = w * (0.92 + 0.16 * u()), h * (0.92 + 0.16 * u())
        return torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)).float()
    a[0] += (u() - 0.5) * 0.16 * a[2]
    a[1] += (u() - 0.5) * 0.16 * a[3]
    a[2] *= 0.92 + 0.16 * u()
    a[3] *= 0.92 + 0.16 * u()
    a[4] += (u() - 0.5) * 6
    return a


def label_margins(q, lo, hi, margin):
    """q (G, R) float64.  -> None when a label hangs on rounding, else the coverage flags.  Deciding IoUs: every anchor's maximum, every
    gt's best (no near-ties with it), and for a positive anchor the gap between its two best gts."""
    vals, best = q.max(0).values, q.max(1).values
    for t in (lo, hi):
        if (vals - t).abs().min() < margin or (best - t).abs().min() < margin:
            return None
    near = (q >= best[:, None] - margin).sum(1)
    if (near != 1).any():
        return None
    lowq = (q == best[:, None]).any(0)
    posit = (vals >= hi) | lowq
    if q.shape[0] > 1:
        top2 = q.topk(2, dim=0).values
        if ((top2[0] - top2[1])[posit] < margin).any():
            return None
    return dict(ignore_band=int(((vals >= lo) & (vals < hi) & ~lowq).sum()), low_quality_only=int(((best >= lo) & (best < hi)).sum()),
                below_low=int((best < lo).sum()), ordinary=int((best >= hi).sum()), positives=int(posit.sum()))


def draw_gts(D, anc, lo, hi, size, seed0):
    """Five gts: two near an anchor (ordinary positives), one whose best IoU lies in the ignore band, one below the low threshold, one
    free; the first seed whose draw meets the margins and the coverage flags."""
    anc64 = anc.double()
    for seed in range(seed0, seed0 + 400):
        g = torch.Generator().manual_seed(seed)
        out = []
        for kind in ("hi", "hi", "band", "low", "any"):
            for _ in range(4000):
                b = _near_anchor(g, anc, D) if kind == "hi" else _rand_box(g, D, size)
                best = float(iou_matrix(b[None].double(), anc64).max())
                if {"hi": best >= hi + 0.03, "band": lo + 0.01 <= best <= hi - 0.01, "low": 0.03 < best <= lo - 0.05, "any": True}[kind]:
                    out.append(b)
                    break
            else:
                raise AssertionError(kind)
        gts = torch.stack(out)
        flags = label_margins(iou_matrix(gts.double(), anc64), lo, hi, MARGIN[D])
        if flags and flags["ignore_band"] >= 1 and flags["low_quality_only"] >= 1 and flags["below_low"] >= 1 and flags["ordinary"] >= 2:
            return gts, flags, seed
    raise AssertionError("no seed meets the label margins")


def np32(t):
    return t.detach().numpy()


def save(name, arrays, meta, line):
    """np.savez_compressed with fixed zip timestamps: regenerating gives the same bytes."""
    path = os.path.join(OUT, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())
    meta[name] = line
    print(f"{name}: {os.path.getsize(path)} bytes")


def both(fn):
    """fn(dtype) -> dict of tensors.  Integer outputs must agree between the fp32 and the float64 run; float outputs are stored twice."""
    r32, r64 = fn(F32), fn(F64)
    out = {}
    for k, v in r32.items():
        if v.dtype.is_floating_point:
            out[k], out[k + "_f64"] = np32(v), np32(r64[k])
        else:
            assert torch.equal(v, r64[k]), f"{k}: the fp32 and float64 runs of the reference disagree on a decision"
            out[k] = np32(v)
    return out


# ------------------------------------------------------------------------------------------------ (a) RetinaNet labels
def retina_labels(retina, D, meta):
    tag = "xyxy" if D == 4 else "rot"
    anc_l = anchors_for(D)
    anc = torch.cat(anc_l)
    gts, flags, seed = draw_gts(D, anc, 0.4, 0.5, IMAGE_SIZES[0], 100 * D)
    gtb = [gts, torch.zeros((0, D))]
    gtc = [torch.tensor([1, 4, 0, 3, 2]), torch.zeros((0,), dtype=torch.int64)]

    def run(dt):
        self = NS(anchor_matcher=Matcher([0.4, 0.5], [0, -1, 1], True), num_classes=K)
        inst = [GT(gt_boxes=Boxes(b.to(dt)), gt_classes=c.clone()) for b, c in zip(gtb, gtc)]
        labels, boxes = retina.RetinaNet.label_anchors(self, [Boxes(a.to(dt)) for a in anc_l], inst)
        return {"gt_labels": torch.stack(labels), "matched_boxes": torch.stack(boxes)}

    out = both(run)
    lab = out["gt_labels"]
    assert (lab[1] == K).all() and (lab[0] == -1).sum() == flags["ignore_band"] and ((lab[0] >= 0) & (lab[0] < K)).sum() == flags["positives"]
    out.update(hw=np.array(HW), strides=np.array(STRIDES), thresholds=np.array([0.4, 0.5]), iou_labels=np.array([0, -1, 1]),
               num_classes=np.array(K), anchors=np32(anc), gt_boxes0=np32(gtb[0]), gt_boxes1=np32(gtb[1]),
               gt_classes0=np32(gtc[0]), gt_classes1=np32(gtc[1]), flags=np.array(json.dumps(flags)))
    save(f"retina_labels_{tag}.npz", out, meta,
         f"(a) reference-Python x restated-op: retina/retina_rotated.py:251-295 label_anchors x restated pairwise_iou ({D} columns) / Matcher; seed {seed}, {flags}")
    return anc_l, torch.from_numpy(out["gt_labels"]), torch.from_numpy(out["matched_boxes"])


# ------------------------------------------------------------------------------------------------ (b) RetinaNet losses
def retina_losses(retina, D, kind, anc_l, gt_labels, matched, meta):
    tag = "xyxy" if D == 4 else "rot"
    g = torch.Generator().manual_seed(7000 + 10 * D + len(kind))
    raw_logits = [torch.randn(N, A * K, h, w, generator=g) * 2.0 - 2.0 for h, w in HW]
    raw_deltas = [torch.randn(N, A * D, h, w, generator=g) * (0.5 if kind == "giou" else 0.3) for h, w in HW]
    weights = W4 if D == 4 else W5
    beta = 0.1
    for d in raw_deltas:       # no |delta| on the scale clamp (the GIoU branch decodes)
        assert ((d / 1.0 - SCALE_CLAMP).abs() > 1e-3).all()

    def run(dt):
        self = NS(num_classes=K, box2box_transform=B2B(weights), loss_normalizer=100, loss_normalizer_momentum=0.9, focal_loss_alpha=0.25,
                  focal_loss_gamma=2.0, smooth_l1_loss_beta=beta, box_reg_loss_type=kind)
        rl = [x.to(dt).requires_grad_(True) for x in raw_logits]
        rd = [x.to(dt).requires_grad_(True) for x in raw_deltas]
        pl = [retina.permute_to_N_HWA_K(x, K) for x in rl]
        pd = [retina.permute_to_N_HWA_K(x, D) for x in rd]
        losses = retina.RetinaNet.losses(self, [Boxes(a.to(dt)) for a in anc_l], pl, list(gt_labels), pd, [m.to(dt) for m in matched])
        gc = torch.autograd.grad(losses["loss_cls"], rl, retain_graph=True)
        gb = torch.autograd.grad(losses["loss_box_reg"], rd)
        res = {"loss_cls": losses["loss_cls"].detach(), "loss_box_reg": losses["loss_box_reg"].detach(),
               "normalizer_after": torch.tensor(float(self.loss_normalizer), dtype=dt)}
        for l in range(len(HW)):
            res[f"logits_perm{l}"], res[f"deltas_perm{l}"] = pl[l].detach(), pd[l].detach()
            res[f"grad_logits{l}"], res[f"grad_deltas{l}"] = gc[l], gb[l]
        return res

    out = both(run)
    pos = (gt_labels >= 0) & (gt_labels != K)
    assert abs(float(out["normalizer_after"]) - (0.9 * 100 + 0.1 * int(pos.sum()))) < 1e-4 and int(pos.sum()) > 1
    assert float(out["loss_box_reg"]) > 0 and float(out["loss_cls"]) > 0
    for l in range(len(HW)):
        out[f"raw_logits{l}"], out[f"raw_deltas{l}"] = np32(raw_logits[l]), np32(raw_deltas[l])
    out.update(anchors=np32(torch.cat(anc_l)), gt_labels=np32(gt_labels), matched_boxes=np32(matched), normalizer_before=np.array(100.0),
               momentum=np.array(0.9), alpha=np.array(0.25), gamma=np.array(2.0), beta=np.array(beta), weights=np.array(weights),
               hw=np.array(HW), num_classes=np.array(K), num_anchors=np.array(A))
    save(f"retina_losses_{kind}_{tag}.npz", out, meta,
         f"(b) reference-Python x restated-op: retina/retina_rotated.py:25-34 permute_to_N_HWA_K, :185-249 losses ({kind}) x restated "
         f"Box2BoxTransform{'Rotated' if D == 5 else ''} / focal / {'giou_loss' if kind == 'giou' else 'smooth_l1_loss'}; autograd gradients")


# ------------------------------------------------------------------------------------------------ (c) RetinaNet inference
def _distinct_topk(scores, k):
    top = scores.sort(descending=True).values[: k + 1]
    return torch.unique(top).numel() == top.numel()


def cap_case(retina, anc_l, weights, topk, thr, nms_thr):
    """Rotated boxes, the last level alone (18 anchors, 90 scores, most above the threshold), one image, a cut wider than the candidates:
    the detections are at most 18, and would be more if the top-k were capped by the level's scores instead of its anchors (:345)."""
    anc, max_det = anc_l[-1], 60
    for seed in range(8500, 8700):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(len(anc), K, generator=g) * 1.2 + 1.5
        deltas = torch.randn(len(anc), 5, generator=g) * 0.1
        p = logits.flatten().sigmoid()
        if not (_distinct_topk(p, len(anc)) and (p - thr).abs().min() > 1e-6 and int((p > thr).sum()) > topk):
            continue
        try:
            NMS_LOG.clear()

            def run(dt):
                self = NS(topk_candidates=topk, score_threshold=thr, num_classes=K, box2box_transform=B2B(weights), nms_threshold=nms_thr,
                          max_detections_per_image=max_det)
                r = retina.RetinaNet.inference_single_image(self, [Boxes(anc.to(dt))], [logits.to(dt).clone()], [deltas.to(dt)], IMAGE_SIZES[0])
                return {"cap_boxes": r.pred_boxes.tensor, "cap_scores": r.scores, "cap_classes": r.pred_classes}

            out = both(run)
        except AssertionError as e:
            print(f"  retina_inference_rot cap case: seed {seed} rejected ({e})")
            continue
        assert all(m == len(anc) for m, _ in NMS_LOG) and len(out["cap_scores"]) <= len(anc) < topk < max_det
        # coverage only (restated): the same with the top-k capped by the level's SCORES must give other detections
        prob, idx = p.sort(descending=True)
        prob, idx = prob[:topk], idx[:topk]
        idx, prob = idx[prob > thr], prob[prob > thr]
        B = orc.apply_deltas(deltas[idx // K], anc[idx // K], weights).view(-1, 5)
        alt = prob[orc.batched_nms_any(B, prob, idx % K, nms_thr)[:max_det]]
        if not np.array_equal(alt.numpy(), out["cap_scores"]):
            out.update(cap_logits=np32(logits), cap_deltas=np32(deltas), cap_max_detections=np.array(max_det), cap_seed=np.array(seed))
            return out
    raise AssertionError("no seed meets the cap case's conditions")


def retina_inference(retina, D, anc_l, meta):
    tag = "xyxy" if D == 4 else "rot"
    # 4 columns: the last level's scores rank high and the global cut is wide, so the cap of that level's top-k by its ANCHOR count (:345)
    # shows in the detections (checked below).  5 columns: the global cut (12) hides the cap in the three-level case (few candidates keep
    # the per-pair Python loop of the restated rotated NMS short); cap_case() shows it on the last level alone.
    visible_cap = D == 4
    topk, thr, nms_thr, max_det = 40, 0.6, 0.5, (30 if visible_cap else 12)
    weights = W4 if D == 4 else W5
    for seed in range(8000 + D, 8400):
        g = torch.Generator().manual_seed(seed)
        logits = [torch.randn(N, h * w * A, K, generator=g) * 1.6 - 0.6 + torch.tensor([0.0, 1.5, 0.0, 0.8, 0.0]) for h, w in HW]
        deltas = [torch.randn(N, h * w * A, D, generator=g) * 0.25 for h, w in HW]
        logits[1] -= 2.2                  # few of this level's scores pass the threshold: it removes some of the top-k
        if visible_cap:
            logits[2] += 2.0
        deltas[0][0, 5, 2] = 5.0          # past the scale clamp
        logits[0][0, 5, 1] = 4.0
        ok = all(((d - SCALE_CLAMP).abs() > 1e-3).all() for d in deltas)
        cut = {"topk_bites": False, "anchors_cap": False, "threshold_bites": False}
        for l, lg in enumerate(logits):
            for i in range(N):
                p = lg[i].flatten().sigmoid()
                k = min(topk, lg.shape[1])
                ok = ok and _distinct_topk(p, k)
                kept = int((p.sort(descending=True).values[:k] > thr).sum())
                ok = ok and ((p - thr).abs().min() > 1e-6)
                cut["topk_bites"] |= lg.shape[1] > topk and kept == k
                cut["anchors_cap"] |= lg.shape[1] < topk and int((p > thr).sum()) > k
                cut["threshold_bites"] |= 0 < kept < k
        if not (ok and all(cut.values())):
            continue
        try:
            NMS_LOG.clear()

            def run(dt):
                self = NS(topk_candidates=topk, score_threshold=thr, num_classes=K, box2box_transform=B2B(weights), nms_threshold=nms_thr,
                          max_detections_per_image=max_det)
                res = {}
                for i in range(N):
                    r = retina.RetinaNet.inference_single_image(self, [Boxes(a.to(dt)) for a in anc_l], [x[i].to(dt).clone() for x in logits],
                                                                [x[i].to(dt) for x in deltas], IMAGE_SIZES[i])
                    res[f"boxes{i}"], res[f"scores{i}"], res[f"classes{i}"] = r.pred_boxes.tensor, r.scores, r.pred_classes
                return res

            out = both(run)
        except AssertionError as e:
            print(f"  retina_inference_{tag}: seed {seed} rejected ({e})")
            continue
        if not all(m > s > max_det for m, s in NMS_LOG):       # NMS suppresses something, and the global cut bites, in every call
            continue
        # coverage only (restated): capping a level's top-k by its anchor x class SCORES instead of its anchors must change the detections
        differs = []
        for i in range(N):
            B, S, C = [], [], []
            for anc, lg, dl in zip(anc_l, logits, deltas):
                prob, idx = lg[i].flatten().sigmoid().sort(descending=True)
                prob, idx = prob[:topk], idx[:topk]
                idx = idx[prob > thr]
                B.append(orc.apply_deltas(dl[i][idx // K], anc[idx // K], weights).view(-1, D)); S.append(prob[prob > thr]); C.append(idx % K)
            B, S, C = torch.cat(B), torch.cat(S), torch.cat(C)
            alt = S[orc.batched_nms_any(B, S, C, nms_thr)[:max_det]]
            differs.append(not np.array_equal(alt.numpy(), out[f"scores{i}"]))
        if all(differs) or not visible_cap:
            break
    else:
        raise AssertionError("no seed meets the inference conditions")
    for i in range(N):
        assert len(out[f"scores{i}"]) == max_det
    if not visible_cap:
        out.update(cap_case(retina, anc_l, weights, topk, thr, nms_thr))
    for l in range(len(HW)):
        out[f"logits{l}"], out[f"deltas{l}"] = np32(logits[l]), np32(deltas[l])
        out[f"anchors{l}"] = np32(anc_l[l])
    out.update(hw=np.array(HW), topk_candidates=np.array(topk), score_threshold=np.array(thr), nms_threshold=np.array(nms_thr),
               max_detections=np.array(max_det), weights=np.array(weights), image_sizes=np.array(IMAGE_SIZES), num_classes=np.array(K),
               nms_candidates_survivors=np.array(NMS_LOG))
    save(f"retina_inference_{tag}.npz", out, meta,
         f"(c) reference-Python x restated-op: retina/retina_rotated.py:319-378 inference_single_image x restated "
         f"Box2BoxTransform{'Rotated' if D == 5 else ''}.apply_deltas / batched_nms ({D} columns) / Instances; seed {seed}, NMS (candidates, survivors) {NMS_LOG}")


# ------------------------------------------------------------------------------------------------ (d) RPN labels, sampling, losses
def rpn_labels_losses(rpn, D, meta):
    tag = "xyxy" if D == 4 else "rot"
    anc_l = anchors_for(D)
    anc = torch.cat(anc_l)
    S, frac = 16, 0.5
    weights = RPN_W4 if D == 4 else RPN_W5
    gts, flags, seed = draw_gts(D, anc, 0.3, 0.7, IMAGE_SIZES[0], 300 * D)
    gtb = [gts, torch.zeros((0, D))]
    g = torch.Generator().manual_seed(9000 + D)
    raw_logits = [torch.randn(N, A, h, w, generator=g) * 2.0 for h, w in HW]
    raw_deltas = [torch.randn(N, A * D, h, w, generator=g) * 0.3 for h, w in HW]
    R = RPNWNM = rpn.RPNWNM

    def run(dt):
        SAMPLER.seen, SAMPLER.gen = [], torch.Generator().manual_seed(41)
        self = NS(anchor_matcher=Matcher([0.3, 0.7], [0, -1, 1], True), anchor_boundary_thresh=-1.0, batch_size_per_image=S,
                  positive_fraction=frac, box2box_transform=B2B(weights), in_features=["p3", "p4", "p5"], training=False)
        self._subsample_labels = lambda label: R._subsample_labels(self, label)
        ancb = [Boxes(a.to(dt)) for a in anc_l]
        labels, boxes = R.label_and_sample_anchors(self, ancb, [GT(gt_boxes=Boxes(b.to(dt)), image_size=s) for b, s in zip(gtb, IMAGE_SIZES)])
        res = {"labels_before_sampling": torch.stack(SAMPLER.seen), "labels_sampled": torch.stack(labels), "matched_boxes": torch.stack(boxes)}
        # the two reshapes of forward (:278-289): the head gives raw tensors, predict_proposals receives the reshaped ones
        got = {}
        self.anchor_generator = lambda feats: ancb
        self.anchor_generator.box_dim = D
        rl = [x.to(dt).requires_grad_(True) for x in raw_logits]
        rd = [x.to(dt).requires_grad_(True) for x in raw_deltas]
        self.rpn_head = lambda feats: (rl, rd)
        self.predict_proposals = lambda a, lg, dl, sizes: got.update(lg=lg, dl=dl)
        R.forward(self, NS(image_sizes=IMAGE_SIZES), {"p3": None, "p4": None, "p5": None})
        for l in range(len(HW)):
            res[f"logits_perm{l}"], res[f"deltas_perm{l}"] = got["lg"][l].detach(), got["dl"][l].detach()
        for name, beta in (("beta0", 0.0), ("beta02", 0.2)):
            self.smooth_l1_beta = beta
            losses = R.losses(self, ancb, got["lg"], labels, got["dl"], boxes)
            gc = torch.autograd.grad(losses["loss_rpn_cls"], rl, retain_graph=True)
            gl = torch.autograd.grad(losses["loss_rpn_loc"], rd, retain_graph=True)
            res[f"loss_rpn_cls_{name}"], res[f"loss_rpn_loc_{name}"] = losses["loss_rpn_cls"].detach(), losses["loss_rpn_loc"].detach()
            for l in range(len(HW)):
                res[f"grad_logits{l}_{name}"], res[f"grad_deltas{l}_{name}"] = gc[l], gl[l]
        return res

    out = both(run)
    before, after = out["labels_before_sampling"], out["labels_sampled"]
    assert (before[1] == 0).all() and (before[0] == -1).sum() == flags["ignore_band"] and (before[0] == 1).sum() == flags["positives"]
    assert ((after == 1).sum(1) == np.minimum((before == 1).sum(1), int(S * frac))).all() and ((after >= 0).sum(1) == S).all()
    assert (after[0] == 1).sum() >= 2 and ((after == -1) & (before == 0)).any() and (before[after >= 0] == after[after >= 0]).all()
    d = orc.get_deltas(anc, torch.from_numpy(out["matched_boxes"][0]), weights)[torch.from_numpy(after[0] == 1)]
    pred = torch.cat([torch.from_numpy(out[f"deltas_perm{l}"][0]) for l in range(3)])[torch.from_numpy(after[0] == 1)]
    assert ((pred - d).abs() < 0.2).any() and ((pred - d).abs() > 0.2).any(), "both smooth-L1 branches must be exercised"
    for l in range(len(HW)):
        out[f"raw_logits{l}"], out[f"raw_deltas{l}"] = np32(raw_logits[l]), np32(raw_deltas[l])
    out.update(anchors=np32(anc), gt_boxes0=np32(gtb[0]), gt_boxes1=np32(gtb[1]), thresholds=np.array([0.3, 0.7]), iou_labels=np.array([0, -1, 1]),
               batch_size_per_image=np.array(S), positive_fraction=np.array(frac), weights=np.array(weights), hw=np.array(HW),
               normalizer=np.array(S * N), image_sizes=np.array(IMAGE_SIZES), num_anchors=np.array(A), flags=np.array(json.dumps(flags)))
    save(f"rpn_labels_losses_{tag}.npz", out, meta,
         f"(d) reference-Python x restated-op: proposal_generator/rpn.py:118-134 _subsample_labels, :136-191 label_and_sample_anchors, :193-251 losses, "
         f":278-289 reshapes of forward x restated pairwise_iou ({D} columns) / Matcher / Box2BoxTransform{'Rotated' if D == 5 else ''} / "
         f"smooth_l1_loss, recording subsample_labels stub; seed {seed}, {flags}")


# ------------------------------------------------------------------------------------------------ (e) proposals
def rpn_proposals(rpn, putils, D, meta):
    tag = "xyxy" if D == 4 else "rot"
    anc_l = anchors_for(D)
    weights = RPN_W4 if D == 4 else RPN_W5
    nms_thr, min_side = 0.7, 4.0
    cfgs = {"train": (True, 30, 25), "eval": (False, 20, 12), "nonfinite": (False, 20, 12)}
    pick = 1                           # level-0 anchors at cell (0, 0) (x = 0 border); rotated: the angle-0 anchor
    for seed in range(9500 + D, 9900):
        g = torch.Generator().manual_seed(seed)
        logits = [torch.randn(N, h * w * A, generator=g) * 2.0 for h, w in HW]
        deltas = [torch.randn(N, h * w * A, D, generator=g) * 0.3 for h, w in HW]
        for i in range(N):       # boxes that become small only through clipping: pushed out over the left border, high logit
            deltas[0][i, pick] = torch.tensor([(-0.30 if D == 4 else -0.40) - 0.02 * i, 0.1, 0.05, 0.1] + ([0.002] if D == 5 else []))
            logits[0][i, pick] = 5.0 + i
            # a pair NMS decides: the neighbour cell's anchor moved onto this one (IoU ~0.8 > 0.7), both with high logits
            deltas[1][i, 3 * 7 + 1], deltas[1][i, 3 * 8 + 1] = torch.zeros(D), torch.tensor([-0.4 if D == 4 else -0.28, 0.02, 0.03, -0.02] + ([0.01] if D == 5 else []))
            logits[1][i, 3 * 7 + 1], logits[1][i, 3 * 8 + 1] = 3.5 + 0.1 * i, 3.2 + 0.1 * i
        deltas[1][0, 7, 3] = 5.0          # past the scale clamp
        logits[1][0, 7] = 4.5
        if not all(((d[..., 2:4] - SCALE_CLAMP).abs() > 1e-3).all() for d in deltas):
            continue
        if not all(torch.unique(lg[i]).numel() == lg.shape[1] for lg in logits for i in range(N)):
            continue
        bad_d = [d.clone() for d in deltas]
        bad_l = [x.clone() for x in logits]
        top0 = logits[0][0].sort(descending=True).indices
        bad_d[0][0, top0[3], 1] = float("nan")
        bad_l[0][0, top0[5]] = float("inf")
        try:
            out, NMS_LOG[:] = {}, []
            extra = {}
            for name, (training, pre, post) in cfgs.items():
                lg_in, dl_in = (bad_l, bad_d) if name == "nonfinite" else (logits, deltas)

                def run(dt):
                    self = NS(box2box_transform=B2B(weights))
                    ancb = [Boxes(a.to(dt)) for a in anc_l]
                    props = rpn.RPNWNM._decode_proposals(self, ancb, [d.to(dt) for d in dl_in])
                    # proposal_utils.py:75 indexes anchors.unsqueeze(0) with the batch index: the function only runs on one image at a time
                    res = [putils.find_top_rpn_proposals_anchors(ancb, [p[i:i + 1] for p in props], [x[i:i + 1].to(dt) for x in lg_in], IMAGE_SIZES[i:i + 1],
                                                                 nms_thr, pre, post, min_side, training)[0] for i in range(N)]
                    o = {f"decoded{l}": p for l, p in enumerate(props)}
                    for i, r in enumerate(res):
                        o[f"proposal_boxes{i}"], o[f"anchor_boxes{i}"], o[f"objectness_logits{i}"] = r.proposal_boxes.tensor, r.anchor_boxes.tensor, r.objectness_logits
                        o[f"count{i}"] = torch.tensor(len(r.proposal_boxes))
                    return o

                mark = len(NMS_LOG)
                for k, v in both(run).items():
                    out[f"{name}_{k}"] = v
                calls = NMS_LOG[mark:mark + N]          # the fp32 run's calls
                assert all(s > post for _, s in calls), "post_nms_topk must cut"
                assert all(m > s for m, s in calls), "NMS must suppress something"
                extra[name] = calls
                # clipping before the small-box filter: sides within 1e-3 of min_side are excluded, and the crafted boxes are removed
                for i in range(N):
                    P = torch.cat([torch.from_numpy(out[f"{name}_decoded{l}_f64"][i]) for l in range(3)])
                    P = P[torch.isfinite(P).all(1)]
                    c = orc.clip_boxes(P, IMAGE_SIZES[i])
                    side = (lambda b: torch.stack((b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), 1) if D == 4 else b[:, 2:4])
                    assert ((side(c) - min_side).abs() > 1e-3).all(), "a clipped side sits on min_box_side_len"
                    small_by_clip = (side(c).min(1).values <= min_side) & (side(P).min(1).values > min_side)
                    assert small_by_clip.any(), "no box becomes small through clipping alone"
            assert int(out["nonfinite_count0"]) > 0
        except AssertionError as e:
            print(f"  rpn_proposals_{tag}: seed {seed} rejected ({e})")
            continue
        break
    else:
        raise AssertionError("no seed meets the proposal conditions")
    # the crafted boxes are in every level-0 top-k and in no output
    for name in cfgs:
        for i in range(N):
            assert not (out[f"{name}_objectness_logits{i}"] == 5.0 + i).any()
    assert not np.isfinite(out["nonfinite_decoded0"][0]).all() and np.isfinite(out["nonfinite_proposal_boxes0"]).all()
    for l in range(len(HW)):
        out[f"logits{l}"], out[f"deltas{l}"], out[f"anchors{l}"] = np32(logits[l]), np32(deltas[l]), np32(anc_l[l])
        out[f"nonfinite_logits{l}"], out[f"nonfinite_deltas{l}"] = np32(bad_l[l]), np32(bad_d[l])
    out.update(hw=np.array(HW), image_sizes=np.array(IMAGE_SIZES), nms_thresh=np.array(nms_thr), min_box_side_len=np.array(min_side),
               weights=np.array(weights), cfg=np.array(json.dumps({k: [bool(v[0]), v[1], v[2]] for k, v in cfgs.items()})), num_anchors=np.array(A))
    save(f"rpn_proposals_{tag}.npz", out, meta,
         f"(e) reference-Python x restated-op: proposal_generator/rpn.py:337-356 _decode_proposals, proposal_generator/proposal_utils.py:11-130 "
         f"find_top_rpn_proposals_anchors x restated Box2BoxTransform{'Rotated' if D == 5 else ''}.apply_deltas / Boxes.clip / Boxes.nonempty / "
         f"batched_nms ({D} columns) / Instances; one image per call (:75 indexes a batch of one); training, eval and eval with a NaN box and an inf score; seed {seed}, NMS (candidates, survivors) {extra}")


# ------------------------------------------------------------------------------------------------ (f) Fast R-CNN inference
def fast_rcnn_inference(frcnn, meta):
    Rn, thr, nms_thr = 48, 0.25, 0.5
    size = IMAGE_SIZES[0]
    for seed in range(9900, 10300):
        g = torch.Generator().manual_seed(seed)
        cx, cy = torch.rand(Rn, generator=g) * 70 + 5, torch.rand(Rn, generator=g) * 54 + 5
        w, h = torch.rand(Rn, generator=g) * 30 + 8, torch.rand(Rn, generator=g) * 30 + 8
        props = torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), 1)
        anchors = props + torch.randn(Rn, 4, generator=g) * 2
        boxes_k = (props[:, None] + torch.randn(Rn, K, 4, generator=g) * 3).reshape(Rn, K * 4)
        boxes_1 = props + torch.randn(Rn, 4, generator=g) * 3
        scores = torch.softmax(torch.randn(Rn, K + 1, generator=g) * 2.0, 1)
        boxes_k[11, 6] = float("nan")
        boxes_1[11, 2] = float("inf")
        if (scores[:, :-1] - thr).abs().min() < 1e-6:
            continue
        try:
            out, NMS_LOG[:] = {}, []
            for name, bx, topk in (("specific_top10", boxes_k, 10), ("specific_all", boxes_k, -1), ("agnostic_top10", boxes_1, 10), ("agnostic_all", boxes_1, -1)):
                def run(dt):
                    p = Instances(size)
                    p.anchor_boxes, p.proposal_boxes = Boxes(anchors.to(dt)), Boxes(props.to(dt))
                    r, rows = frcnn.fast_rcnn_inference_single_image_with_anchor(p, bx.to(dt), scores.to(dt), size, thr, nms_thr, topk)
                    return {"boxes": r.pred_boxes.tensor, "scores": r.scores, "classes": r.pred_classes, "rows_of_finite_input": rows,
                            "anchors": r.anchors.tensor, "proposals": r.proposals.tensor}

                for k, v in both(run).items():
                    out[f"{name}_{k}"] = v
            assert all(m > s for m, s in NMS_LOG) and all(s > 10 for _, s in NMS_LOG), NMS_LOG
        except AssertionError as e:
            print(f"  fast_rcnn_inference: seed {seed} rejected ({e})")
            continue
        break
    else:
        raise AssertionError("no seed meets the Fast R-CNN inference conditions")
    assert len(out["specific_top10_scores"]) == 10 and len(out["specific_all_scores"]) > 10 and int((scores[:, :-1] > thr).sum()) > len(out["specific_all_scores"])
    out.update(proposal_boxes=np32(props), anchor_boxes=np32(anchors), boxes_specific=np32(boxes_k), boxes_agnostic=np32(boxes_1), probs=np32(scores),
               image_size=np.array(size), score_thresh=np.array(thr), nms_thresh=np.array(nms_thr), num_classes=np.array(K))
    save("fast_rcnn_inference.npz", out, meta,
         f"(f) reference-Python x restated-op: roi_heads/fast_rcnn.py:53-115 fast_rcnn_inference_single_image_with_anchor x restated Boxes.clip / "
         f"batched_nms / Instances; class-specific (R, K*4) and class-agnostic (R, 4) boxes, topk 10 and -1, one non-finite row; seed {seed}")


def main():
    assert os.path.isdir(REF), "runs only where the reference tree exists (/root/reference)"
    torch.set_num_threads(1)
    retina, rpn, putils, frcnn = install()
    meta = {}
    for D in (4, 5):
        anc_l, labels, matched = retina_labels(retina, D, meta)
        retina_losses(retina, D, "smooth_l1", anc_l, labels, matched, meta)
        if D == 4:
            retina_losses(retina, D, "giou", anc_l, labels, matched, meta)
        retina_inference(retina, D, anc_l, meta)
        rpn_labels_losses(rpn, D, meta)
        rpn_proposals(rpn, putils, D, meta)
    fast_rcnn_inference(frcnn, meta)
    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    biggest = max(os.path.getsize(os.path.join(OUT, "..", n)) for n in os.listdir(os.path.join(OUT, "..")) if n.endswith(".npz"))
    assert all(os.path.getsize(os.path.join(OUT, n)) <= biggest for n in meta)


if __name__ == "__main__":
    main()
