// Minimum-area enclosing rectangles of polygon annotations on device, in float64: the geometry behind the reference's oriented ratio
// (COCO.compute_ratio, PolygonMasks.get_ratios(oriented=True), concern.support.ratio_of_polygon) and its rotated ground truth
// (COCO.compute_rbox, concern.support.rbox_from_polygon, tools/mask_to_rbox.py), which call OpenCV's convexHull + minAreaRect.
// Host side: slenderobjdet_amd/structures/polygons.py, whose numpy path restates the same arithmetic operation by operation.
//
// One wave64 per annotation, four per 256-thread block, waves striding over the annotations; a wave never waits for another one, so
// the kernel holds no block barrier.  The points of an annotation with at most SOD_POLYGON_LDS_POINTS points are staged in the wave's
// LDS slice, larger ones are read from global memory (L2) on every pass.
//
// Hull by gift wrapping from the lexicographically smallest point: every step is one wave-wide arg-reduction ("the point no other
// point lies to the right of, the farthest of collinear ones"), which yields the vertices counter-clockwise without collinear ones,
// the order of coco_gt._hull.  The rectangle of the edge just found needs the extents of the points along the edge and its normal:
// a second reduction, over all points (the hull is never stored: no workspace).  Cost O(n * hull vertices).  The walk is bounded:
// it stops after n steps whatever the orientation tests say, and every other loop runs over n points.
#include <math.h>

#include "common.h"
#include "../../include/slender_hip.h"

namespace {

constexpr int PG_WAVES = 4;                           // annotations (waves) per block
constexpr int PG_LDS = SOD_POLYGON_LDS_POINTS;        // points of one wave's LDS slice
constexpr int PG_MAX_POINTS = SOD_POLYGON_MAX_POINTS;
constexpr double PG_DEG = 57.29577951308232;          // 180 / pi

struct PtsGlobal {
  const double2* p;
  __device__ __forceinline__ double2 operator()(int i) const { return p[i]; }
};
struct PtsLds {
  const double* x;
  const double* y;
  __device__ __forceinline__ double2 operator()(int i) const { return make_double2(x[i], y[i]); }
};

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// Gift-wrapping order around the current vertex c: r replaces the candidate q when it lies to the right of c -> q, or on that line and
// farther from c.  A candidate equal to c (the start value, and every copy of c) has a zero offset: it loses to any other point and
// beats none, so it needs no flag.
__device__ __forceinline__ void wrap_pick(double cx, double cy, double& qx, double& qy, double rx, double ry) {
  const double ax = qx - cx, ay = qy - cy, bx = rx - cx, by = ry - cy;
  const double cr = ax * by - ay * bx;
  if (cr < 0.0 || (cr == 0.0 && bx * bx + by * by > ax * ax + ay * ay)) {
    qx = rx;
    qy = ry;
  }
}

template <class Pts>
__device__ void min_area_rect_wave(const Pts P, const int n, const int lane, double* __restrict__ rect, int* __restrict__ info) {
  const double inf = __builtin_huge_val();
  // the lexicographically smallest point and the axis-aligned extent
  double sx = inf, sy = inf, lox = inf, hix = -inf, loy = inf, hiy = -inf;
  for (int i = lane; i < n; i += 64) {
    const double2 p = P(i);
    if (p.x < sx || (p.x == sx && p.y < sy)) {
      sx = p.x;
      sy = p.y;
    }
    lox = fmin(lox, p.x);
    hix = fmax(hix, p.x);
    loy = fmin(loy, p.y);
    hiy = fmax(hiy, p.y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ox = __shfl_xor(sx, o, 64), oy = __shfl_xor(sy, o, 64);
    if (ox < sx || (ox == sx && oy < sy)) {
      sx = ox;
      sy = oy;
    }
  }
  sx = __shfl(sx, 0, 64);
  sy = __shfl(sy, 0, 64);
  lox = wave_min_f64(lox);
  hix = wave_max_f64(hix);
  loy = wave_min_f64(loy);
  hiy = wave_max_f64(hiy);

  double cx = sx, cy = sy;
  int hull = 1;                // distinct points met so far: 1, then the vertices of the closed walk
  bool have = false;
  double best_area = 0.0, b_ux = 1.0, b_uy = 0.0, b_lou = 0.0, b_hiu = 0.0, b_lov = 0.0, b_hiv = 0.0;
  for (int step = 0; step < n; ++step) {          // at most n edges
    double qx = cx, qy = cy;
    for (int i = lane; i < n; i += 64) {
      const double2 p = P(i);
      wrap_pick(cx, cy, qx, qy, p.x, p.y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wrap_pick(cx, cy, qx, qy, __shfl_xor(qx, o, 64), __shfl_xor(qy, o, 64));
    qx = __shfl(qx, 0, 64);    // one answer for the wave even where rounding makes the order inconsistent
    qy = __shfl(qy, 0, 64);
    if (qx == cx && qy == cy) break;              // every point coincides with c
    hull = step + 1;
    const double ex = qx - cx, ey = qy - cy;
    const double len = sqrt(ex * ex + ey * ey);
    if (len > 0.0) {
      const double ux = ex / len, uy = ey / len;
      double lou = inf, hiu = -inf, lov = inf, hiv = -inf;
      for (int i = lane; i < n; i += 64) {
        const double2 p = P(i);
        const double pu = p.x * ux + p.y * uy, pv = p.y * ux - p.x * uy;
        lou = fmin(lou, pu);
        hiu = fmax(hiu, pu);
        lov = fmin(lov, pv);
        hiv = fmax(hiv, pv);
      }
      lou = wave_min_f64(lou);
      hiu = wave_max_f64(hiu);
      lov = wave_min_f64(lov);
      hiv = wave_max_f64(hiv);
      const double area = (hiu - lou) * (hiv - lov);
      if (!have || area < best_area) {            // strict: the first minimal edge wins a tie
        have = true;
        best_area = area;
        b_ux = ux; b_uy = uy; b_lou = lou; b_hiu = hiu; b_lov = lov; b_hiv = hiv;
      }
    }
    cx = qx;
    cy = qy;
    if (cx == sx && cy == sy) break;              // closed
  }

  double o0, o1, o2, o3, o4;
  if (hull < 3 || !have) {     // one point, coincident or collinear points: the axis-aligned extent
    if (hull >= 3) hull = 2;
    o0 = (lox + hix) / 2;
    o1 = (loy + hiy) / 2;
    o2 = hix - lox;
    o3 = hiy - loy;
    o4 = 0.0;
  } else {
    const double mu = (b_lou + b_hiu) / 2, mv = (b_lov + b_hiv) / 2;
    o0 = b_ux * mu - b_uy * mv;
    o1 = b_uy * mu + b_ux * mv;
    double w = b_hiu - b_lou, h = b_hiv - b_lov;
    // detectron2's angle (width axis (cos a, -sin a) in image coordinates), folded into (-45, 45]
    double a = atan2(-b_uy, b_ux) * PG_DEG;
    int k = (int)ceil((a - 45.0) / 90.0);
    a -= 90.0 * k;
    if (a > 45.0) {
      a -= 90.0;
      ++k;
    } else if (a <= -45.0) {
      a += 90.0;
      --k;
    }
    if (k & 1) {
      const double t = w;
      w = h;
      h = t;
    }
    o2 = w;
    o3 = h;
    o4 = a + 0.0;              // -0 -> +0
  }
  if (lane == 0) {
    rect[0] = o0;
    rect[1] = o1;
    rect[2] = o2;
    rect[3] = o3;
    rect[4] = o4;
    *info = hull;
  }
}

__global__ __launch_bounds__(64 * PG_WAVES) void polygon_min_area_rect_kernel(const double* __restrict__ xy, const int* __restrict__ ann_off,
                                                                              int A, double* __restrict__ rect, int* __restrict__ info) {
  __shared__ double s_x[PG_WAVES][PG_LDS];
  __shared__ double s_y[PG_WAVES][PG_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long stride = (long long)gridDim.x * PG_WAVES;
  for (long long a = (long long)blockIdx.x * PG_WAVES + wave; a < A; a += stride) {
    const int p0 = ann_off[a];
    const int n = ann_off[a + 1] - p0;
    double* r = rect + 5 * a;
    if (n <= 0 || n > PG_MAX_POINTS || p0 < 0) {  // nothing to enclose / beyond the supported size: the host refuses these
      if (lane < 5) r[lane] = n == 0 ? 0.0 : __builtin_nan("");
      if (lane == 0) info[a] = n == 0 ? 0 : -1;
      continue;
    }
    const double2* src = reinterpret_cast<const double2*>(xy) + p0;
    if (n <= PG_LDS) {
      for (int i = lane; i < n; i += 64) {
        const double2 p = src[i];
        s_x[wave][i] = p.x;
        s_y[wave][i] = p.y;
      }
      // the slice belongs to this wave alone: its LDS accesses complete in order, the fence keeps the compiler from moving them
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      min_area_rect_wave(PtsLds{s_x[wave], s_y[wave]}, n, lane, r, info + a);
      // the next annotation's staging must not overtake this one's reads
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    } else {
      min_area_rect_wave(PtsGlobal{src}, n, lane, r, info + a);
    }
  }
}

}  // namespace

extern "C" int sod_polygon_min_area_rect(const double* xy, const int* ann_off, int A, double* rect, int* info, void* stream) {
  if (A < 0 || A > SOD_POLYGON_MAX_ANNS) return SOD_EARG;
  if (A == 0) return SOD_OK;
  if (!xy || !ann_off || !rect || !info) return SOD_EARG;
  if ((uintptr_t)xy & 15) return SOD_EALIGN;      // points are read as 16-byte pairs
  // at least two annotations per wave where there are that many (start-up is paid once), at most four resident blocks per compute unit
  const long long want = ((long long)A + 2 * PG_WAVES - 1) / (2 * PG_WAVES);
  const long long cap = 4LL * device_cus();
  const int blocks = (int)(want < cap ? want : cap);
  SOD_LAUNCH(polygon_min_area_rect_kernel, dim3(blocks), dim3(64 * PG_WAVES), 0, (hipStream_t)stream, xy, ann_off, A, rect, info);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
