// The IoU losses of ONE box pair (GIoU of XYXY boxes, rotated IoU, rotated GIoU) and their gradients w.r.t. the first box, as device code:
// shared by the pair operators (the GiouXyxyPair policy of detection_ops.hip and RotIouPair of rotated_iou_loss.hip, under the skeleton of
// pair_loss.h) and the fused box losses (box_loss_policy.h).  The including file places this header inside its own anonymous namespace (after common.h), like rotated_iou.h.
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

// dI[0..5) = d (intersection area) / d a (angle: per degree); ca, sa, cb, sb = cosf / sinf of the two angles in radians
__device__ __forceinline__ void riou_dinter(const float* a, const float* b, float ca, float sa, float cb, float sb, float* dI) {
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
  dI[0] = (L0 - L1) * ca + (L2 - L3) * sa;             // outward normals: +-ax = +-(ca, -sa), +-ay = +-(sa, ca)
  dI[1] = (L2 - L3) * ca - (L0 - L1) * sa;
  dI[2] = 0.5f * (L0 + L1);
  dI[3] = 0.5f * (L2 + L3);
  dI[4] = (L0 * v0 - L1 * v1 - L2 * u2 + L3 * u3) * RIOU_D2R;
}

// g[0..5) = d (1 - IoU) / d a for a pair with forward IoU ``iou`` > 0 (angle: per degree)
__device__ __forceinline__ void riou_grad(const float* a, const float* b, float iou, float* g) {
  const float ta = a[4] * RIOU_D2R, tb = b[4] * RIOU_D2R;
  float dI[5];
  riou_dinter(a, b, cosf(ta), sinf(ta), cosf(tb), sinf(tb), dI);
  const float w = a[2], h = a[3];
  const float asum = w * h + b[2] * b[3];
  const float inter = iou * asum / (1.f + iou);        // iou = I / (asum - I)
  const float U = asum - inter, rU2 = 1.f / (U * U);
  const float dA[5] = {0.f, 0.f, h, w, 0.f};
#pragma unroll
  for (int e = 0; e < 5; ++e) g[e] = -(dI[e] * U - inter * (dA[e] - dI[e])) * rU2;
}

// ---- rotated GIoU: 1 - IoU + (C - U) / C with C the area of the convex hull of the 8 corners of the two boxes.
// The hull in registers, every index a compile-time constant (a dynamically indexed private array would sit in scratch): the 8 corners,
// relative to the midpoint of the two centres, are sorted by (x, y, target before prediction) with a 19-exchange network; then Andrew's
// two chains as gift-wrapping walks that can only move FORWARD in that order - the lower chain from point 0 to point 7 over larger
// indices, the upper chain back over smaller ones.  From point j the successor is the most clockwise candidate (cross products of the
// differences to j; all candidates of a chain lie in one half plane, so this is an order), and both chains are evaluated for every j, the
// walk being the bit mask of the points it reaches.  Whatever rounding does to a near-tie, the walk is ONE closed polygon through points
// of the set: a nearly collinear point taken or left costs a sliver of the order of the rounding of a cross product, and no edge can be
// dropped or counted twice.  C = 1/2 sum cross(p, q) over the walked edges; the origin lies inside the hull, so no term is negative.
// Ties: of exactly collinear candidates the farthest is the successor, so a point inside a hull edge is no vertex and has no gradient; of
// coincident points the first in the sorted order is the successor, and the walk may pass through the other by an edge of length 0.  The
// gradient is that of the shoelace sum over the walked vertex sequence - at a tie a one-sided derivative (the side on which the walked
// vertices stay the hull's).
struct HullPts { float x[8], y[8], su[8], sv[8]; };      // su, sv = +-1: the corner c + su*(w/2)*ax + sv*(h/2)*ay of a; 0, 0: a corner of b

__device__ __forceinline__ void hull_exchange(HullPts& p, int i, int j) {
  const bool sw = p.x[i] > p.x[j] || (p.x[i] == p.x[j] && (p.y[i] > p.y[j] || (p.y[i] == p.y[j] && p.su[i] != 0.f && p.su[j] == 0.f)));
  const float x = p.x[i], y = p.y[i], su = p.su[i], sv = p.sv[i];
  p.x[i] = sw ? p.x[j] : x; p.y[i] = sw ? p.y[j] : y; p.su[i] = sw ? p.su[j] : su; p.sv[i] = sw ? p.sv[j] : sv;
  p.x[j] = sw ? x : p.x[j]; p.y[j] = sw ? y : p.y[j]; p.su[j] = sw ? su : p.su[j]; p.sv[j] = sw ? sv : p.sv[j];
}

// sums of the vertex gradients of a's corners, weighted by 1, su and sv: all the chain rule to (cx, cy, w, h, angle) needs
struct HullGrad { float gx, gy, ux, uy, vx, vy; };
__device__ __forceinline__ void hull_vertex_grad(HullGrad& G, float su, float sv, float gx, float gy) {
  const float m = su * su;
  G.gx += m * gx; G.gy += m * gy;
  G.ux += su * gx; G.uy += su * gy;
  G.vx += sv * gx; G.vy += sv * gy;
}

// One step of a chain: the successor of point J among the points [K0, K1) and, if the walk ``on`` has reached J, its edge.
template <bool GRAD, int J, int K0, int K1>
__device__ __forceinline__ void hull_step(const HullPts& p, unsigned& on, float& area2, HullGrad& G) {
  float bdx = 0.f, bdy = 0.f, bd2 = 0.f, bx = p.x[J], by = p.y[J], bsu = p.su[J], bsv = p.sv[J];
  int bi = J;
#pragma unroll
  for (int k = K0; k < K1; ++k) {
    const float dx = p.x[k] - p.x[J], dy = p.y[k] - p.y[J];
    const float c = bdx * dy - bdy * dx, d2 = dx * dx + dy * dy;
    const bool take = c < 0.f || (c == 0.f && d2 > bd2);
    bdx = take ? dx : bdx; bdy = take ? dy : bdy; bd2 = take ? d2 : bd2;
    bx = take ? p.x[k] : bx; by = take ? p.y[k] : by; bi = take ? k : bi;
    if (GRAD) { bsu = take ? p.su[k] : bsu; bsv = take ? p.sv[k] : bsv; }
  }
  if ((on >> J) & 1u) {
    on |= 1u << bi;
    area2 += p.x[J] * by - p.y[J] * bx;
    if (GRAD) {
      hull_vertex_grad(G, p.su[J], p.sv[J], by, -bx);
      hull_vertex_grad(G, bsu, bsv, -p.y[J], p.x[J]);
    }
  }
}

// -> C, the hull area of the boxes a and b; if GRAD, dC[0..5) = d C / d a (angle: per degree)
template <bool GRAD>
__device__ __forceinline__ float hull_area(const float* a, const float* b, float ca, float sa, float cb, float sb, float* dC) {
  const float hx = 0.5f * (a[0] - b[0]), hy = 0.5f * (a[1] - b[1]);      // a's centre relative to the midpoint; b's is the negative
  const float hw = 0.5f * a[2], hh = 0.5f * a[3], hwb = 0.5f * b[2], hhb = 0.5f * b[3];
  HullPts p;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float su = (k == 0 || k == 1) ? 1.f : -1.f, sv = (k == 0 || k == 3) ? 1.f : -1.f;
    p.x[k] = -hx + su * hwb * cb + sv * hhb * sb; p.y[k] = -hy - su * hwb * sb + sv * hhb * cb; p.su[k] = 0.f; p.sv[k] = 0.f;
    p.x[4 + k] = hx + su * hw * ca + sv * hh * sa; p.y[4 + k] = hy - su * hw * sa + sv * hh * ca; p.su[4 + k] = su; p.sv[4 + k] = sv;
  }
  hull_exchange(p, 0, 2); hull_exchange(p, 1, 3); hull_exchange(p, 4, 6); hull_exchange(p, 5, 7);
  hull_exchange(p, 0, 4); hull_exchange(p, 1, 5); hull_exchange(p, 2, 6); hull_exchange(p, 3, 7);
  hull_exchange(p, 0, 1); hull_exchange(p, 2, 3); hull_exchange(p, 4, 5); hull_exchange(p, 6, 7);
  hull_exchange(p, 2, 4); hull_exchange(p, 3, 5);
  hull_exchange(p, 1, 4); hull_exchange(p, 3, 6);
  hull_exchange(p, 1, 2); hull_exchange(p, 3, 4); hull_exchange(p, 5, 6);
  float area2 = 0.f;
  HullGrad G{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  unsigned on = 1u;                    // the lower chain: from point 0 over larger indices
  hull_step<GRAD, 0, 1, 8>(p, on, area2, G); hull_step<GRAD, 1, 2, 8>(p, on, area2, G); hull_step<GRAD, 2, 3, 8>(p, on, area2, G);
  hull_step<GRAD, 3, 4, 8>(p, on, area2, G); hull_step<GRAD, 4, 5, 8>(p, on, area2, G); hull_step<GRAD, 5, 6, 8>(p, on, area2, G);
  hull_step<GRAD, 6, 7, 8>(p, on, area2, G);
  on = 1u << 7;                        // the upper chain: from point 7 over smaller ones
  hull_step<GRAD, 7, 0, 7>(p, on, area2, G); hull_step<GRAD, 6, 0, 6>(p, on, area2, G); hull_step<GRAD, 5, 0, 5>(p, on, area2, G);
  hull_step<GRAD, 4, 0, 4>(p, on, area2, G); hull_step<GRAD, 3, 0, 3>(p, on, area2, G); hull_step<GRAD, 2, 0, 2>(p, on, area2, G);
  hull_step<GRAD, 1, 0, 1>(p, on, area2, G);
  if (GRAD) {
    dC[0] = 0.5f * G.gx;
    dC[1] = 0.5f * G.gy;
    dC[2] = 0.25f * (G.ux * ca - G.uy * sa);
    dC[3] = 0.25f * (G.vx * sa + G.vy * ca);
    dC[4] = 0.5f * (hh * (G.vx * ca - G.vy * sa) - hw * (G.ux * sa + G.uy * ca)) * RIOU_D2R;
  }
  return 0.5f * area2;
}

// The rotated GIoU loss of one pair with forward IoU ``iou`` (iou_rotated_lds; I and U are recovered from it as in riou_grad; iou == 0:
// I = 0, U = the two areas, dI = 0) -> 1 - iou + (C - U) / C; if GRAD, g = its gradient w.r.t. a, the IoU part being riou_grad's.
// C <= 0 (both boxes degenerate): no hull term and no gradient of it.  The rounding of C - U is clamped at 0 in the value.  GRAD is a
// template parameter: a g chosen at run time ("d ? g : nullptr") would force the caller's array out of its registers into scratch.
template <bool GRAD>
__device__ __forceinline__ float rgiou_pair(const float* a, const float* b, float iou, float* g) {
  const float ta = a[4] * RIOU_D2R, tb = b[4] * RIOU_D2R;
  const float ca = cosf(ta), sa = sinf(ta), cb = cosf(tb), sb = sinf(tb);
  const float asum = a[2] * a[3] + b[2] * b[3];
  const float inter = iou * asum / (1.f + iou);
  const float U = asum - inter;
  float dC[5];
  const float C = hull_area<GRAD>(a, b, ca, sa, cb, sb, dC);
  const bool hull = C > 0.f;
  if (GRAD) {
    float dI[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (iou > 0.f) riou_dinter(a, b, ca, sa, cb, sb, dI);
    const float rU2 = 1.f / (U * U), rC2 = 1.f / (C * C);
    const float dA[5] = {0.f, 0.f, a[3], a[2], 0.f};
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const float dU = dA[e] - dI[e];
      const float gi = iou > 0.f ? -(dI[e] * U - inter * dU) * rU2 : 0.f;
      g[e] = gi + (hull ? (U * dC[e] - C * dU) * rC2 : 0.f);
    }
  }
  return (1.f - iou) + (hull ? fmaxf(C - U, 0.f) / C : 0.f);
}
