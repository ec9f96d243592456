// detectron2's Box2BoxTransform (XYXY boxes) and Box2BoxTransformRotated ((cx, cy, w, h, angle_deg) boxes) as device code: ONE definition
// for rcnn_ops.hip (sod_box2box_*), detection_ops.hip (retina_targets_kernel), rotated_retina.hip (the labeller, the decode) and
// retina_box_loss.hip (the GIoU / rotated IoU policies).  The including file places this header inside its own anonymous namespace (after
// common.h), like rotated_iou.h; the library is built with -ffp-contract=off, so every site gets the same bits out of these functions.
// s / t / d / b are anything indexable by [e] (a pointer, a float array, an f32x4_t); o is a float array or pointer.
#pragma once

constexpr float SOD_PI = 3.14159265358979323846f;

struct W5 { float w[5]; };      // the transform's weights: (wx, wy, ww, wh) of XYXY boxes, plus the angle's weight of rotated ones

// host side: the first D weights, each of which must be positive
inline bool fill_w5(W5& w, const float* weights, int D = 5) {
  if (!weights) return false;
  for (int i = 0; i < D; ++i) {
    if (!(weights[i] > 0.f)) return false;
    w.w[i] = weights[i];
  }
  return true;
}

// The two clamps of dw / dh that live in this library.  For a finite delta they agree; for a NaN delta they do not:
//   CLAMP_DROPS_NAN  fminf(dw, clampv)           -> clampv: the NaN is gone (rcnn_ops.hip, retina_decode_rot_kernel - which zeroes non-finite
//                                                   boxes afterwards, so the difference is observable there -, the rotated IoU loss)
//   CLAMP_KEEPS_NAN  dw > clampv ? clampv : dw   -> NaN: the box and its loss are NaN (the GIoU loss)
enum ClampForm { CLAMP_DROPS_NAN, CLAMP_KEEPS_NAN };
template <ClampForm F>
__device__ __forceinline__ float clamp_delta(float d, float clampv) {
  if constexpr (F == CLAMP_KEEPS_NAN) return d > clampv ? clampv : d;
  else return fminf(d, clampv);
}

// ---- Box2BoxTransform (XYXY)
template <class S, class T>
__device__ __forceinline__ void xyxy_get_deltas(const S& s, const T& t, const float* w, float* o) {
  const float sw = s[2] - s[0], sh = s[3] - s[1], scx = s[0] + 0.5f * sw, scy = s[1] + 0.5f * sh;
  const float tw = t[2] - t[0], th = t[3] - t[1], tcx = t[0] + 0.5f * tw, tcy = t[1] + 0.5f * th;
  o[0] = w[0] * (tcx - scx) / sw; o[1] = w[1] * (tcy - scy) / sh;
  o[2] = w[2] * logf(tw / sw); o[3] = w[3] * logf(th / sh);
}

// what a backward chain rule through apply_deltas needs besides the box: the source box's and the decoded widths, and whether dw / dh
// were clamped (a clamped width has no gradient)
struct XyxyDecoded { float bw, bh, pw, ph; bool cw, ch; };
template <ClampForm F, class D, class B>
__device__ __forceinline__ XyxyDecoded xyxy_apply_deltas(const D& d, const B& b, const float* w, float clampv, float* o) {
  XyxyDecoded r;
  r.bw = b[2] - b[0]; r.bh = b[3] - b[1];
  const float cx = b[0] + 0.5f * r.bw, cy = b[1] + 0.5f * r.bh;
  const float dx = d[0] / w[0], dy = d[1] / w[1], dw = d[2] / w[2], dh = d[3] / w[3];
  r.cw = dw > clampv; r.ch = dh > clampv;
  const float pcx = dx * r.bw + cx, pcy = dy * r.bh + cy;
  r.pw = expf(clamp_delta<F>(dw, clampv)) * r.bw; r.ph = expf(clamp_delta<F>(dh, clampv)) * r.bh;
  o[0] = pcx - 0.5f * r.pw; o[1] = pcy - 0.5f * r.ph; o[2] = pcx + 0.5f * r.pw; o[3] = pcy + 0.5f * r.ph;
  return r;
}

// ---- Box2BoxTransformRotated (cx, cy, w, h, angle in degrees)
template <class S, class T>
__device__ __forceinline__ void rot_get_deltas(const S& s, const T& t, const float* w, float* o) {
  o[0] = w[0] * (t[0] - s[0]) / s[2]; o[1] = w[1] * (t[1] - s[1]) / s[3];
  o[2] = w[2] * logf(t[2] / s[2]); o[3] = w[3] * logf(t[3] / s[3]);
  float da = t[4] - s[4];
  da = fmodf(da + 180.f, 360.f);
  if (da < 0.f) da += 360.f;            // python's % (result takes the sign of the divisor)
  da -= 180.f;
  o[4] = da * w[4] * SOD_PI / 180.f;
}

// the decoded widths are o[2] and o[3]; every site clamps with CLAMP_DROPS_NAN
struct RotDecoded { bool cw, ch; };
template <class D, class B>
__device__ __forceinline__ RotDecoded rot_apply_deltas(const D& d, const B& b, const float* w, float clampv, float* o) {
  const float dx = d[0] / w[0], dy = d[1] / w[1], dw = d[2] / w[2], dh = d[3] / w[3];
  const float da = d[4] / w[4];
  o[0] = dx * b[2] + b[0]; o[1] = dy * b[3] + b[1];
  o[2] = expf(clamp_delta<CLAMP_DROPS_NAN>(dw, clampv)) * b[2]; o[3] = expf(clamp_delta<CLAMP_DROPS_NAN>(dh, clampv)) * b[3];
  float a = da * 180.f / SOD_PI + b[4];
  a = fmodf(a + 180.f, 360.f);
  if (a < 0.f) a += 360.f;
  o[4] = a - 180.f;
  return RotDecoded{dw > clampv, dh > clampv};
}
