// The IoU losses of ONE box pair and their gradients w.r.t. the first box, as device code: shared by the pair operators
// (giou_xyxy_kernel of detection_ops.hip, rotated_iou_loss_kernel of rotated_iou_loss.hip) and the fused RetinaNet box loss
// (retina_box_loss.hip).  The including file places this header inside its own anonymous namespace (after common.h), like rotated_iou.h.
#pragma once

// fvcore giou_loss of one XYXY pair; g (may be null): its gradient w.r.t. a.  max/min ties split like torch.
template <class A, class B>
__device__ __forceinline__ float giou_pair(const A& a, const B& b, float eps, float* g) {
  const float x1 = a[0], y1 = a[1], x2 = a[2], y2 = a[3], x1g = b[0], y1g = b[1], x2g = b[2], y2g = b[3];
  const float xk1 = fmaxf(x1, x1g), yk1 = fmaxf(y1, y1g), xk2 = fminf(x2, x2g), yk2 = fminf(y2, y2g);
  const bool ov = (yk2 > yk1) && (xk2 > xk1);
  const float inter = ov ? (xk2 - xk1) * (yk2 - yk1) : 0.f;
  const float uni = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter;
  const float iou = inter / (uni + eps);
  const float xc1 = fminf(x1, x1g), yc1 = fminf(y1, y1g), xc2 = fmaxf(x2, x2g), yc2 = fmaxf(y2, y2g);
  const float ac = (xc2 - xc1) * (yc2 - yc1);
  if (g) {
    // derivatives of inter / union / hull w.r.t. (x1,y1,x2,y2) of box a
    auto dmax = [](float p, float q) { return p > q ? 1.f : (p == q ? 0.5f : 0.f); };
    auto dmin = [](float p, float q) { return p < q ? 1.f : (p == q ? 0.5f : 0.f); };
    const float iw = xk2 - xk1, ih = yk2 - yk1, w1 = x2 - x1, h1 = y2 - y1, cw = xc2 - xc1, ch = yc2 - yc1;
    const float di[4] = {ov ? -dmax(x1, x1g) * ih : 0.f, ov ? -dmax(y1, y1g) * iw : 0.f, ov ? dmin(x2, x2g) * ih : 0.f, ov ? dmin(y2, y2g) * iw : 0.f};
    const float da[4] = {-h1, -w1, h1, w1};
    const float dc[4] = {-dmin(x1, x1g) * ch, -dmin(y1, y1g) * cw, dmax(x2, x2g) * ch, dmax(y2, y2g) * cw};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float du = da[e] - di[e];
      const float diou = (di[e] * (uni + eps) - inter * du) / ((uni + eps) * (uni + eps));
      const float dterm = ((dc[e] - du) * (ac + eps) - (ac - uni) * dc[e]) / ((ac + eps) * (ac + eps));
      g[e] = -(diou - dterm);
    }
  }
  return 1.f - (iou - (ac - uni) / (ac + eps));
}

// ---- 1 - IoU of rotated boxes (cx, cy, w, h, angle_deg): the gradient.  The forward value is iou_rotated_lds of rotated_iou.h; the
// derivation is at the head of rotated_iou_loss.hip.
constexpr float RIOU_D2R = 0.01745329251994329577f;

// The part [t0, t1] of the segment p(t) = (x0, y0) + t * (x1 - x0, y1 - y0), t in [0, 1], inside |x| <= hx, |y| <= hy:
// -> t1 - t0 (0 when empty) and the midpoint parameter.
__device__ __forceinline__ void clip_to_slabs(float x0, float y0, float x1, float y1, float hx, float hy, float& frac, float& tm) {
  float t0 = 0.f, t1 = 1.f;
  {
    const float d = x1 - x0;
    if (d == 0.f) { if (fabsf(x0) > hx) { t0 = 2.f; t1 = -1.f; } }
    else {
      const float ta = (-hx - x0) / d, tb = (hx - x0) / d;
      t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
    }
  }
  {
    const float d = y1 - y0;
    if (d == 0.f) { if (fabsf(y0) > hy) { t0 = 2.f; t1 = -1.f; } }
    else {
      const float ta = (-hy - y0) / d, tb = (hy - y0) / d;
      t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
    }
  }
  frac = fmaxf(t1 - t0, 0.f);
  tm = 0.5f * (t0 + t1);
}

// g[0..5) = d (1 - IoU) / d a for a pair with forward IoU ``iou`` > 0 (angle: per degree)
__device__ __forceinline__ void riou_grad(const float* a, const float* b, float iou, float* g) {
  const float ta = a[4] * RIOU_D2R, tb = b[4] * RIOU_D2R;
  const float ca = cosf(ta), sa = sinf(ta), cb = cosf(tb), sb = sinf(tb);
  const float w = a[2], h = a[3], hw = 0.5f * w, hh = 0.5f * h, hwb = 0.5f * b[2], hhb = 0.5f * b[3];
  const float dx = a[0] - b[0], dy = a[1] - b[1];
  // centre and axes of a in the frame of b
  const float cxl = dx * cb - dy * sb, cyl = dx * sb + dy * cb;
  const float axx = ca * cb + sa * sb, axy = ca * sb - sa * cb, ayx = -axy, ayy = axx;
  const float wx = hw * axx, wy = hw * axy, hx = hh * ayx, hy = hh * ayy;       // half extents as vectors
  float f0, m0, f1, m1, f2, m2, f3, m3;
  clip_to_slabs(cxl + wx - hx, cyl + wy - hy, cxl + wx + hx, cyl + wy + hy, hwb, hhb, f0, m0);      // u = +w/2, v from -h/2 to +h/2
  clip_to_slabs(cxl - wx - hx, cyl - wy - hy, cxl - wx + hx, cyl - wy + hy, hwb, hhb, f1, m1);      // u = -w/2
  clip_to_slabs(cxl - wx + hx, cyl - wy + hy, cxl + wx + hx, cyl + wy + hy, hwb, hhb, f2, m2);      // v = +h/2, u from -w/2 to +w/2
  clip_to_slabs(cxl - wx - hx, cyl - wy - hy, cxl + wx - hx, cyl + wy - hy, hwb, hhb, f3, m3);      // v = -h/2
  const float L0 = f0 * h, L1 = f1 * h, L2 = f2 * w, L3 = f3 * w;
  const float v0 = m0 * h - hh, v1 = m1 * h - hh, u2 = m2 * w - hw, u3 = m3 * w - hw;
  float dI[5];
  dI[0] = (L0 - L1) * ca + (L2 - L3) * sa;             // outward normals: +-ax = +-(ca, -sa), +-ay = +-(sa, ca)
  dI[1] = (L2 - L3) * ca - (L0 - L1) * sa;
  dI[2] = 0.5f * (L0 + L1);
  dI[3] = 0.5f * (L2 + L3);
  dI[4] = (L0 * v0 - L1 * v1 - L2 * u2 + L3 * u3) * RIOU_D2R;
  const float asum = w * h + b[2] * b[3];
  const float inter = iou * asum / (1.f + iou);        // iou = I / (asum - I)
  const float U = asum - inter, rU2 = 1.f / (U * U);
  const float dA[5] = {0.f, 0.f, h, w, 0.f};
#pragma unroll
  for (int e = 0; e < 5; ++e) g[e] = -(dI[e] * U - inter * (dA[e] - dI[e])) * rU2;
}
