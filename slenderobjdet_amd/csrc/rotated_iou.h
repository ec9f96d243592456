// Rotated-box IoU as device code, shared by nms.hip, detection_ops.hip (anchor labelling, pairwise IoU) and coco_eval_rotated.hip.
// The including file places this header inside its own anonymous namespace (after common.h); the library is built with
// -ffp-contract=off, so every translation unit gets the same bits out of these functions.
#pragma once

// ---- rotated boxes (cx, cy, w, h, angle_deg): detectron2 box_iou_rotated ----
struct P2 { float x, y; };
__device__ __forceinline__ P2 psub(P2 a, P2 b) { return P2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ float pcross(P2 a, P2 b) { return a.x * b.y - b.x * a.y; }
__device__ __forceinline__ float pdot(P2 a, P2 b) { return a.x * b.x + a.y * b.y; }

__device__ __forceinline__ void rot_vertices(float cx, float cy, float w, float h, float cs, float sn, P2* pts) {
  const float c2 = cs * 0.5f, s2 = sn * 0.5f;      // cs / sn = cosf / sinf of the angle in radians (computed once by the caller)
  pts[0] = P2{cx + s2 * h + c2 * w, cy + c2 * h - s2 * w};
  pts[1] = P2{cx - s2 * h + c2 * w, cy - c2 * h - s2 * w};
  pts[2] = P2{2.f * cx - pts[0].x, 2.f * cy - pts[0].y};
  pts[3] = P2{2.f * cx - pts[1].x, 2.f * cy - pts[1].y};
}

// Where the up-to-24 candidate points of the clipping live.  A private array is indexed dynamically and therefore sits in SCRATCH memory
// (400 B per lane): the bubble sort and the Graham scan below then make a few hundred trips to memory per box pair - measured ~50 000 cycles
// per pair and lane.  The hot kernels hand in a slice of LDS instead (point k of thread t at [k * stride + t]).
struct RotPtsPrivate {
  P2 v[24];
  __device__ __forceinline__ P2 get(int i) const { return v[i]; }
  __device__ __forceinline__ void set(int i, P2 p) { v[i] = p; }
};
struct RotPtsLds {
  P2* base; int stride;
  __device__ __forceinline__ P2 get(int i) const { return base[i * stride]; }
  __device__ __forceinline__ void set(int i, P2 p) { base[i * stride] = p; }
};

// detectron2's rotated-box intersection (box_iou_rotated_utils.h), the same candidate points, the same bubble sort by polar angle and the
// same Graham scan in the same order - the result must match the reference's to the bit wherever a threshold decides a label or a keep.
template <class PTS>
__device__ __forceinline__ float rot_intersection_area(const P2* p1, const P2* p2, PTS& q) {
  int num = 0;
  P2 v1[4], v2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { v1[i] = psub(p1[(i + 1) & 3], p1[i]); v2[i] = psub(p2[(i + 1) & 3], p2[i]); }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float det = pcross(v2[j], v1[i]);
      if (fabsf(det) <= 1e-14f) continue;
      const P2 v12 = psub(p2[j], p1[i]);
      const float t1 = pcross(v2[j], v12) / det, t2 = pcross(v1[i], v12) / det;
      if (t1 >= 0.f && t1 <= 1.f && t2 >= 0.f && t2 <= 1.f) q.set(num++, P2{p1[i].x + v1[i].x * t1, p1[i].y + v1[i].y * t1});
    }
  {
    const P2 AB = v2[0], DA = v2[3];
    const float ABAB = pdot(AB, AB), ADAD = pdot(DA, DA);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const P2 AP = psub(p1[i], p2[0]);
      const float apab = pdot(AP, AB), apad = -pdot(AP, DA);
      if (apab >= 0.f && apad >= 0.f && apab <= ABAB && apad <= ADAD) q.set(num++, p1[i]);
    }
  }
  {
    const P2 AB = v1[0], DA = v1[3];
    const float ABAB = pdot(AB, AB), ADAD = pdot(DA, DA);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const P2 AP = psub(p2[i], p1[0]);
      const float apab = pdot(AP, AB), apad = -pdot(AP, DA);
      if (apab >= 0.f && apad >= 0.f && apab <= ABAB && apad <= ADAD) q.set(num++, p2[i]);
    }
  }
  if (num <= 2) return 0.f;
  // Graham scan
  int t = 0;
  {
    P2 best = q.get(0);
    for (int i = 1; i < num; ++i) {
      const P2 c = q.get(i);
      if (c.y < best.y || (c.y == best.y && c.x < best.x)) { t = i; best = c; }
    }
    // q[i] = inter[i] - start, in place, then q[0] <-> q[t]
    for (int i = 0; i < num; ++i) q.set(i, psub(q.get(i), best));
    const P2 tmp = q.get(0); q.set(0, q.get(t)); q.set(t, tmp);
  }
  for (int i = 1; i < num - 1; ++i) {        // bubble sort by polar angle around q[0] (as the CUDA path of detectron2)
    P2 cur = q.get(1);
    for (int j = 1; j < num - i; ++j) {
      const P2 nxt = q.get(j + 1);
      const float c = pcross(cur, nxt);
      const bool swap = (c < -1e-6f) || (fabsf(c) < 1e-6f && pdot(cur, cur) > pdot(nxt, nxt));
      if (swap) { q.set(j, nxt); }            // cur moves up to j + 1
      else { q.set(j, cur); cur = nxt; }
    }
    q.set(num - i, cur);
  }
  int k = 1;
  for (; k < num; ++k) {
    const P2 c = q.get(k);
    if (pdot(c, c) > 1e-8f) break;
  }
  if (k == num) return 0.f;
  q.set(1, q.get(k));
  int m = 2;
  for (int i = k + 1; i < num; ++i) {
    const P2 qi = q.get(i);
    while (m > 1) {
      const P2 b2 = q.get(m - 2);
      if (pcross(psub(qi, b2), psub(q.get(m - 1), b2)) >= 0.f) --m; else break;
    }
    q.set(m++, qi);
  }
  if (m <= 2) return 0.f;
  float area = 0.f;
  const P2 q0 = q.get(0);
  P2 prev = q.get(1);
  for (int i = 1; i < m - 1; ++i) {
    const P2 nx = q.get(i + 1);
    area += fabsf(pcross(psub(prev, q0), psub(nx, q0)));
    prev = nx;
  }
  return area / 2.f;
}

template <class PTS>
__device__ __forceinline__ float iou_rotated_impl(const float* a, const float* b, PTS& pts) {
  const float area1 = a[2] * a[3], area2 = b[2] * b[3];
  if (area1 < 1e-14f || area2 < 1e-14f) return 0.f;
  {   // disjoint circumscribed circles => empty intersection => IoU exactly 0 (skips the polygon clipping for almost every pair)
    const float dx = a[0] - b[0], dy = a[1] - b[1];
    const float ra = 0.5f * sqrtf(a[2] * a[2] + a[3] * a[3]), rb = 0.5f * sqrtf(b[2] * b[2] + b[3] * b[3]);
    const float rs = ra + rb;
    if (dx * dx + dy * dy > rs * rs * 1.0001f) return 0.f;
  }
  const float tha = a[4] * 0.01745329251994329577f, thb = b[4] * 0.01745329251994329577f;
  const float ca = cosf(tha), sa = sinf(tha), cb = cosf(thb), sb = sinf(thb);
  {   // Separating-axis test on the four face normals (w axis (cos, -sin), h axis (sin, cos) as in rot_vertices): rectangles separated by a
      // margin have no edge crossing and no contained vertex, so the clipping below returns EXACTLY 0 - provided its own arithmetic cannot
      // invent a crossing: a computed crossing point is off by ~eps * |p2 - p1| / sin(angle between the edges), which stays below the
      // margin unless the edges are within ~1 degree of parallel.  Hence only for boxes at least a pixel thick whose axes are more than
      // ~3 degrees from parallel / perpendicular; everything else takes the full computation as before.
    const float c = ca * cb + sa * sb, s2 = sa * cb - ca * sb;        // cos / sin of (angle a - angle b)
    const float ac = fabsf(c), as = fabsf(s2);
    if (ac > 0.05f && as > 0.05f && fminf(fminf(a[2], a[3]), fminf(b[2], b[3])) >= 1.f) {
      const float dx = b[0] - a[0], dy = b[1] - a[1];
      const float m = 0.05f + 1e-4f * (a[2] + a[3] + b[2] + b[3]);
      const float hwa = 0.5f * a[2], hha = 0.5f * a[3], hwb = 0.5f * b[2], hhb = 0.5f * b[3];
      if (fabsf(dx * ca - dy * sa) > hwa + hwb * ac + hhb * as + m) return 0.f;
      if (fabsf(dx * sa + dy * ca) > hha + hwb * as + hhb * ac + m) return 0.f;
      if (fabsf(dx * cb - dy * sb) > hwb + hwa * ac + hha * as + m) return 0.f;
      if (fabsf(dx * sb + dy * cb) > hhb + hwa * as + hha * ac + m) return 0.f;
    }
  }
  const float sx = (a[0] + b[0]) / 2.f, sy = (a[1] + b[1]) / 2.f;   // centre shift for precision
  P2 p1[4], p2[4];
  rot_vertices(a[0] - sx, a[1] - sy, a[2], a[3], ca, sa, p1);
  rot_vertices(b[0] - sx, b[1] - sy, b[2], b[3], cb, sb, p2);
  const float inter = rot_intersection_area(p1, p2, pts);
  return inter / (area1 + area2 - inter);
}

__device__ float iou_rotated(const float* a, const float* b) {          // candidate points in a private (scratch) array
  RotPtsPrivate pts;
  return iou_rotated_impl(a, b, pts);
}

// candidate points in LDS: ``lds`` = this thread's first slot of a [24][stride] P2 array shared by the ``stride`` threads of the workgroup
__device__ float iou_rotated_lds(const float* a, const float* b, P2* lds, int stride) {
  RotPtsLds pts{lds, stride};
  return iou_rotated_impl(a, b, pts);
}
