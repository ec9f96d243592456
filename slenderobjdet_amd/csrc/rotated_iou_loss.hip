// Rotated IoU box loss: loss = 1 - IoU(pred, target) on (cx, cy, w, h, angle_deg) boxes, with its gradient w.r.t. the prediction.
//   * sod_rotated_iou_loss: the pair operator (the rotated sibling of sod_giou_loss_xyxy).
//   * sod_retina_riou_loss_*: RotatedRetinaNet's BBOX_REG_LOSS_TYPE "rotated_iou" on the pitched delta buffer (the rotated sibling of
//     sod_retina_giou_loss_*): positives decode their five deltas against the anchor (Box2BoxTransformRotated.apply_deltas) and take
//     the pair loss against the matched gt box; the backward pass chains through the decode.
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
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "rotated_iou.h"

constexpr int RL_RED = 1024;
constexpr float RL_PI = 3.14159265358979323846f;
constexpr float RL_D2R = 0.01745329251994329577f;

inline int rl_nblk(long long n, int cap = RL_RED) {
  long long g = (n + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

struct RLW5 { float w[5]; };

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
  const float ta = a[4] * RL_D2R, tb = b[4] * RL_D2R;
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
  dI[4] = (L0 * v0 - L1 * v1 - L2 * u2 + L3 * u3) * RL_D2R;
  const float asum = w * h + b[2] * b[3];
  const float inter = iou * asum / (1.f + iou);        // iou = I / (asum - I)
  const float U = asum - inter, rU2 = 1.f / (U * U);
  const float dA[5] = {0.f, 0.f, h, w, 0.f};
#pragma unroll
  for (int e = 0; e < 5; ++e) g[e] = -(dI[e] * U - inter * (dA[e] - dI[e])) * rU2;
}

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
    const float l = 1.f - iou;
    if (elem) elem[i] = l;
    acc += l;
    if (d1) {
      float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (iou > 0.f) riou_grad(a, b, iou, g);
#pragma unroll
      for (int e = 0; e < 5; ++e) d1[i * 5 + e] = g[e] * gs;
    }
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0 && part) part[blockIdx.x] = acc;
}

__global__ void riou_finish_sum_kernel(const float* __restrict__ part, int nblk_, float* __restrict__ out) {
  __shared__ float red[4];
  float v = 0.f;
  for (int i = threadIdx.x; i < nblk_; i += 256) v += part[i];
  v = block_sum_256(v, red);
  if (threadIdx.x == 0) out[0] = v;
}

// ---------------------------------------------------------------------------------------------- the fused RetinaNet form
struct RetinaRiouArgs {
  const float* pred;        // (N, sumHW, pitch) fp32: anchor a of pixel p at p*pitch + a*5
  const int* labels;        // (N, R)
  const float* anchors;     // (R, 5)
  const float* gt;          // (N, R, 5) matched gt boxes
  int N, R, A, pitch, num_classes;
  RLW5 w;
  float clampv;
};

template <bool BWD, typename T = __bf16>      // T: storage type of the delta gradient (bf16 product path, float in the fp32 validation mode)
__global__ __launch_bounds__(256) void retina_riou_kernel(const RetinaRiouArgs a, float* __restrict__ part, const float* __restrict__ gnum,
                                                          const float* __restrict__ gden, T* __restrict__ dpred) {
  __shared__ P2 rot_pts[24 * 256];
  __shared__ float red[4];
  float acc = 0.f, npos = 0.f;
  const float sc = BWD ? gnum[0] / gden[0] : 0.f;
  const long long total = (long long)a.N * a.R, pix_per_img = a.R / a.A;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / a.R, r = i - n * a.R, px = r / a.A;
    const int an = (int)(r - px * a.A);
    const long long po = (n * pix_per_img + px) * a.pitch + an * 5;
    const int lab = a.labels[i];
    const bool pos = lab >= 0 && lab != a.num_classes;
    float gd[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (pos) {
      npos += 1.f;
      float d[5], s[5], t[5], box[5];
#pragma unroll
      for (int e = 0; e < 5; ++e) { d[e] = a.pred[po + e]; s[e] = a.anchors[r * 5 + e]; t[e] = a.gt[i * 5 + e]; }
      // Box2BoxTransformRotated.apply_deltas, as apply_deltas_kernel of rcnn_ops.hip / retina_decode_rot_kernel
      const float ddx = d[0] / a.w.w[0], ddy = d[1] / a.w.w[1], dw = d[2] / a.w.w[2], dh = d[3] / a.w.w[3], da = d[4] / a.w.w[4];
      const bool cw_ = dw > a.clampv, ch_ = dh > a.clampv;
      box[0] = ddx * s[2] + s[0]; box[1] = ddy * s[3] + s[1];
      box[2] = expf(fminf(dw, a.clampv)) * s[2]; box[3] = expf(fminf(dh, a.clampv)) * s[3];
      float ang = da * 180.f / RL_PI + s[4];
      ang = fmodf(ang + 180.f, 360.f);
      if (ang < 0.f) ang += 360.f;
      box[4] = ang - 180.f;
      const float iou = iou_rotated_lds(box, t, rot_pts + threadIdx.x, 256);
      acc += 1.f - iou;
      if (BWD && iou > 0.f) {
        float g[5];
        riou_grad(box, t, iou, g);
        gd[0] = g[0] * s[2] / a.w.w[0];
        gd[1] = g[1] * s[3] / a.w.w[1];
        gd[2] = cw_ ? 0.f : g[2] * box[2] / a.w.w[2];
        gd[3] = ch_ ? 0.f : g[3] * box[3] / a.w.w[3];
        gd[4] = g[4] * 180.f / (RL_PI * a.w.w[4]);
      }
    }
    if (BWD) {
#pragma unroll
      for (int e = 0; e < 5; ++e) dpred[po + e] = (T)(gd[e] * sc);
      if (an == a.A - 1) {              // the pixel's last anchor also clears the pad columns [A*5, pitch)
        for (int c = 5; c < a.pitch - an * 5; ++c) dpred[po + c] = (T)0.f;
      }
    }
  }
  if (!BWD) {
    acc = block_sum_256(acc, red);
    npos = block_sum_256(npos, red);
    if (threadIdx.x == 0) { part[blockIdx.x] = acc; part[RL_RED + blockIdx.x] = npos; }
  }
}

// sums[0] = sum of 1 - IoU over positives, sums[1] = number of positives; normalizer <- m*normalizer + (1-m)*max(npos,1)
__global__ void retina_riou_finish_kernel(const float* __restrict__ part, int nblk_, float* __restrict__ sums, float* __restrict__ normalizer,
                                          float momentum) {
  __shared__ float red[4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nblk_; i += 256) { a += part[i]; b += part[RL_RED + i]; }
  a = block_sum_256(a, red);
  b = block_sum_256(b, red);
  if (threadIdx.x == 0) {
    sums[0] = a; sums[1] = b;
    if (normalizer) normalizer[0] = momentum * normalizer[0] + (1.f - momentum) * fmaxf(b, 1.f);
  }
}

int retina_riou_fill(RetinaRiouArgs& a, const float* pred, int pitch, const int* labels, const float* anchors, const float* gt, int N, int R,
                     int A, int K, const float* w5, float clampv) {
  if (!pred || !labels || !anchors || !gt || !w5 || N <= 0 || R <= 0 || A <= 0 || R % A || pitch < A * 5) return SOD_EARG;
  for (int i = 0; i < 5; ++i) {
    if (!(w5[i] > 0.f)) return SOD_EARG;
    a.w.w[i] = w5[i];
  }
  a.pred = pred; a.labels = labels; a.anchors = anchors; a.gt = gt; a.N = N; a.R = R; a.A = A; a.pitch = pitch; a.num_classes = K;
  a.clampv = clampv;
  return SOD_OK;
}

}  // namespace

extern "C" int sod_rotated_iou_loss(const float* boxes1, const float* boxes2, long long P, float* elem_out, float* sum_out,
                                    const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  if (P < 0 || (P > 0 && (!boxes1 || !boxes2)) || (sum_out && !ws)) return SOD_EARG;      // P == 0: sum_out = 0, nothing else written
  hipStream_t st = (hipStream_t)stream;
  const int g = rl_nblk(P);
  SOD_LAUNCH(rotated_iou_loss_kernel, dim3(g), dim3(256), 0, st, boxes1, boxes2, P, elem_out, sum_out ? ws : nullptr, grad_scale, dboxes1);
  if (sum_out) SOD_LAUNCH(riou_finish_sum_kernel, dim3(1), dim3(256), 0, st, ws, g, sum_out);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_retina_riou_loss_fwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights5, float scale_clamp, float* sums2,
                                        float* normalizer, float momentum, float* ws, void* stream) {
  RetinaRiouArgs a{};
  int rc = retina_riou_fill(a, pred, pitch, gt_labels, anchors, matched_boxes, N, R, A, num_classes, weights5, scale_clamp);
  if (rc || !sums2 || !ws) return rc ? rc : SOD_EARG;
  hipStream_t st = (hipStream_t)stream;
  const int g = rl_nblk((long long)N * R);
  SOD_LAUNCH((retina_riou_kernel<false, __bf16>), dim3(g), dim3(256), 0, st, a, ws, nullptr, nullptr, nullptr);
  SOD_LAUNCH(retina_riou_finish_kernel, dim3(1), dim3(256), 0, st, ws, g, sums2, normalizer, momentum);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_retina_riou_loss_bwd(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                        int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                        const float* grad_num, const float* grad_den, void* dpred_bf16, void* stream) {
  RetinaRiouArgs a{};
  int rc = retina_riou_fill(a, pred, pitch, gt_labels, anchors, matched_boxes, N, R, A, num_classes, weights5, scale_clamp);
  if (rc || !grad_num || !grad_den || !dpred_bf16) return rc ? rc : SOD_EARG;
  SOD_LAUNCH((retina_riou_kernel<true, __bf16>), dim3(rl_nblk((long long)N * R, 4096)), dim3(256), 0, (hipStream_t)stream, a, nullptr, grad_num, grad_den,
             (__bf16*)dpred_bf16);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_retina_riou_loss_bwd_f32(const float* pred, int pitch, const int* gt_labels, const float* anchors, const float* matched_boxes,
                                            int N, int R, int A, int num_classes, const float* weights5, float scale_clamp,
                                            const float* grad_num, const float* grad_den, float* dpred, void* stream) {
  RetinaRiouArgs a{};
  int rc = retina_riou_fill(a, pred, pitch, gt_labels, anchors, matched_boxes, N, R, A, num_classes, weights5, scale_clamp);
  if (rc || !grad_num || !grad_den || !dpred) return rc ? rc : SOD_EARG;
  SOD_LAUNCH((retina_riou_kernel<true, float>), dim3(rl_nblk((long long)N * R, 4096)), dim3(256), 0, (hipStream_t)stream, a, nullptr, grad_num, grad_den, dpred);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
