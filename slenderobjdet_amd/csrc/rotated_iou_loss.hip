// Rotated IoU box loss: loss = 1 - IoU(pred, target) on (cx, cy, w, h, angle_deg) boxes, with its gradient w.r.t. the prediction.
// sod_rotated_iou_loss is the pair operator (the rotated sibling of sod_giou_loss_xyxy): the RotIouPair<false> policy of the pair
// skeleton of pair_loss.h, which owns the loop, the stores and the reduction.  RotatedRetinaNet's BBOX_REG_LOSS_TYPE
// "rotated_iou" on the pitched delta buffer (sod_retina_riou_loss_*) is the RiouLoss policy of retina_box_loss.hip and shares the
// gradient below (riou_grad and clip_to_slabs of box_pair_loss.h).
// Forward: iou_rotated_lds of rotated_iou.h (detectron2's clipping, candidate points in LDS), so the IoU is the very number NMS, the
// matcher and the evaluator see.  Backward: NOT the derivative of that clipping (a sort and a Graham scan) but the boundary form of the
// derivative of the intersection area I of a moving rectangle (the prediction) with a fixed one (the target):
//     dI/dphi = sum over the 4 edges e of the prediction:  L_e * (n_e . V_phi(m_e))
// L_e = length of the part of edge e inside the target (Liang-Barsky against the target's two slabs, in the target's frame), m_e that
// part's midpoint, n_e the outward normal, V_phi the velocity of a boundary point under parameter phi.  With the box axes
// ax = (cos t, -sin t) along w and ay = (sin t, cos t) along h and m = c + u*ax + v*ay:  V_cx = (1, 0), V_cy = (0, 1), V_w = ax*u/w,
// V_h = ay*v/h, V_t = -u*ay + v*ax per radian.  Then with U = w*h + area2 - I:  dIoU = (dI*U - I*dU) / U^2, dU = d(w*h) - dI.
// No dynamically indexed array: the backward pass runs in registers.  A pair whose forward IoU is 0 (disjoint boxes, a degenerate
// area, the early-outs of rotated_iou.h) has NO gradient: five zeros.  Latency-bound fp32 work on a fraction of a percent of the
// anchors, no MFMA.
// sod_rotated_giou_loss (RotIouPair<true>) is the same operator with the hull term: 1 - IoU + (C - U) / C, C the area of the convex hull of the 8 corners
// (rgiou_pair of box_pair_loss.h, where the method and its tie rule are written down; "rotated_giou", the RgiouLoss policy).  The IoU is
// the same call, so the IoU part is unchanged to the bit; a pair without overlap keeps a gradient, the hull term's.
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "rotated_iou.h"
#include "box_pair_loss.h"      // riou_grad, rgiou_pair
#include "pair_loss.h"          // pair_loss_kernel, launch_pairs

template <bool HULL>
struct RotIouPair {
  static constexpr int W = 5;
  using Lds = P2;                             // the clipping's candidate points (see RotPtsLds): 48 KB a block
  static constexpr int LDS_PER_LANE = 24;
  static __device__ __forceinline__ float pair(const float* a, const float* b, float, P2* lds, bool want_grad, float* g) {
    const float iou = iou_rotated_lds(a, b, lds, 256);
    if constexpr (HULL) return want_grad ? rgiou_pair<true>(a, b, iou, g) : rgiou_pair<false>(a, b, iou, nullptr);
    if (want_grad && iou > 0.f) riou_grad(a, b, iou, g);
    return 1.f - iou;
  }
};

}  // namespace

extern "C" int sod_rotated_iou_loss(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out,
                                    const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  return launch_pairs<RotIouPair<false>>(boxes1, boxes2, P, 0.f, elem_out, sum_out, grad_scale, dboxes1, ws, stream);
}
extern "C" int sod_rotated_giou_loss(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out,
                                     const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  return launch_pairs<RotIouPair<true>>(boxes1, boxes2, P, 0.f, elem_out, sum_out, grad_scale, dboxes1, ws, stream);
}
