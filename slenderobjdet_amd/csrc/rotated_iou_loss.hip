// Rotated IoU box loss: loss = 1 - IoU(pred, target) on (cx, cy, w, h, angle_deg) boxes, with its gradient w.r.t. the prediction.
// sod_rotated_iou_loss is the pair operator (the rotated sibling of sod_giou_loss_xyxy); RotatedRetinaNet's BBOX_REG_LOSS_TYPE
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
// sod_rotated_giou_loss is the same operator with the hull term: 1 - IoU + (C - U) / C, C the area of the convex hull of the 8 corners
// (rgiou_pair of box_pair_loss.h, where the method and its tie rule are written down; "rotated_giou", the RgiouLoss policy).  The IoU is
// the same call, so the IoU part is unchanged to the bit; a pair without overlap keeps a gradient, the hull term's.
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "rotated_iou.h"
#include "box_pair_loss.h"      // riou_grad, rgiou_pair

template <bool HULL>
__global__ __launch_bounds__(256) void rotated_iou_loss_kernel(const float* __restrict__ b1, const float* __restrict__ b2, long long P,
                                                               float* __restrict__ elem, float* __restrict__ part,
                                                               const float* __restrict__ gscale, float* __restrict__ d1) {
  __shared__ P2 rot_pts[24 * 256];      // 48 KB: the clipping's candidate points (see RotPtsLds)
  __shared__ float red[4];
  float acc = 0.f;
  const float gs = gscale ? gscale[0] : 1.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    float a[5], b[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) { a[e] = b1[i * 5 + e]; b[e] = b2[i * 5 + e]; }
    const float iou = iou_rotated_lds(a, b, rot_pts + threadIdx.x, 256);
    float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float l;
    if constexpr (HULL) l = d1 ? rgiou_pair<true>(a, b, iou, g) : rgiou_pair<false>(a, b, iou, nullptr);
    else {
      l = 1.f - iou;
      if (d1 && iou > 0.f) riou_grad(a, b, iou, g);
    }
    if (elem) elem[i] = l;
    acc += l;
    if (d1) {
#pragma unroll
      for (int e = 0; e < 5; ++e) d1[i * 5 + e] = g[e] * gs;
    }
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0 && part) part[blockIdx.x] = acc;
}

template <bool HULL>
int launch_pairs(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out, const float* grad_scale, float* dboxes1,
                 float* ws, void* stream) {
  if (P < 0 || (P > 0 && (!boxes1 || !boxes2)) || (sum_out && !ws)) return SOD_EARG;      // P == 0: sum_out = 0, nothing else written
  hipStream_t st = (hipStream_t)stream;
  const int g = sod_nblk(P);
  SOD_LAUNCH(rotated_iou_loss_kernel<HULL>, dim3(g), dim3(256), 0, st, boxes1, boxes2, P, elem_out, sum_out ? ws : nullptr, grad_scale, dboxes1);
  if (sum_out) SOD_LAUNCH(sod_finish_sums_kernel<>, dim3(1), dim3(256), 0, st, ws, g, 1, sum_out, 0);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

}  // namespace

extern "C" int sod_rotated_iou_loss(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out,
                                    const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  return launch_pairs<false>(boxes1, boxes2, P, elem_out, sum_out, grad_scale, dboxes1, ws, stream);
}
extern "C" int sod_rotated_giou_loss(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out,
                                     const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  return launch_pairs<true>(boxes1, boxes2, P, elem_out, sum_out, grad_scale, dboxes1, ws, stream);
}
