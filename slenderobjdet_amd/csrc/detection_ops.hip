// Detection post-/mid-processing operators the reference reaches through detectron2 / torchvision / fvcore
// (sources absent from the reference tree; semantics restated in SURVEY.md Appendix C.3, C.4, C.5, C.13, C.14):
//   roi_align fwd/bwd        detectron2 ROIAlign(aligned=True) used by ROIPooler (roi_heads/roi_heads.py:48-53)
//   roi_align_rotated fwd    detectron2 ROIAlignRotated (configs/rotated/Base-RRCNN-FPN.yaml:31-36)
//   giou / smooth-L1         fvcore.nn.giou_loss / smooth_l1_loss (retina_rotated.py:229,240; rpd.py:389-395): pair policies of pair_loss.h
//   anchor labelling         pairwise_iou + Matcher(thresholds, labels, allow_low_quality_matches) (retina_rotated.py:251-295)
// All are HBM/latency-bound gather kernels: coalesced 16-B channel vectors, wavefront reductions, no MFMA.
#include "common.h"
#include "../../include/slender_hip.h"
#include <stdlib.h>

namespace {

#include "rotated_iou.h"
#include "box_transform.h"      // xyxy_get_deltas
#include "box_pair_loss.h"      // giou_pair
#include "pair_loss.h"          // pair_loss_kernel, launch_pairs

__global__ __launch_bounds__(256) void pairwise_iou_rotated_kernel(const float* __restrict__ b1, int n1, const float* __restrict__ b2, int n2,
                                                                   float* __restrict__ out) {
  __shared__ P2 rot_pts[24 * 256];
  const long long total = (long long)n1 * n2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
    out[i] = iou_rotated_lds(b1 + (i / n2) * 5, b2 + (i % n2) * 5, rot_pts + threadIdx.x, 256);
}

// ---------------------------------------------------------------------------------------------- ROIAlign (aligned=True)
struct RoiArgs {
  const __bf16* x;      // (N,H,W,C) NHWC bf16
  const float* rois;    // (R,5) [batch, x1,y1,x2,y2]  or (R,6) [batch, cx,cy,w,h,angle_deg] when rotated
  int R, N, H, W, C, PH, PW, sampling_ratio;
  float scale;
  int rotated;
};

__device__ __forceinline__ void bilinear_setup(float y, float x, int H, int W, int& yl, int& xl, int& yh, int& xh, float w[4], bool& valid) {
  valid = !(y < -1.0f || y > (float)H || x < -1.0f || x > (float)W);
  if (y <= 0.f) y = 0.f;
  if (x <= 0.f) x = 0.f;
  yl = (int)y; xl = (int)x;
  if (yl >= H - 1) { yh = yl = H - 1; y = (float)yl; } else yh = yl + 1;
  if (xl >= W - 1) { xh = xl = W - 1; x = (float)xl; } else xh = xl + 1;
  const float ly = y - yl, lx = x - xl, hy = 1.f - ly, hx = 1.f - lx;
  w[0] = hy * hx; w[1] = hy * lx; w[2] = ly * hx; w[3] = ly * lx;
}

// one thread = one (roi, ph, pw, 8-channel vector); XF32: the features are fp32 (validation mode, SOD_PRECISION=fp32)
template <bool BWD, bool XF32 = false>
__global__ __launch_bounds__(256) void roi_align_kernel(const RoiArgs a, float* __restrict__ out /* fwd (R,PH,PW,C) f32 */,
                                                        const float* __restrict__ dout, float* __restrict__ dx /* (N,H,W,C) f32 */) {
  const int c8n = a.C >> 3;
  const long long total = (long long)a.R * a.PH * a.PW * c8n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c8 = (int)(i % c8n);
    long long t = i / c8n;
    const int pw = (int)(t % a.PW); t /= a.PW;
    const int ph = (int)(t % a.PH);
    const int r = (int)(t / a.PH);
    const float* roi = a.rois + (long long)r * (a.rotated ? 6 : 5);
    const int b = (int)roi[0];
    float start_h, start_w, roi_h, roi_w, cth = 1.f, sth = 0.f, ctr_h = 0.f, ctr_w = 0.f;
    if (a.rotated) {
      ctr_w = roi[1] * a.scale - 0.5f; ctr_h = roi[2] * a.scale - 0.5f;
      roi_w = roi[3] * a.scale; roi_h = roi[4] * a.scale;
      const float theta = roi[5] * 3.14159265358979323846f / 180.0f;
      cth = cosf(theta); sth = sinf(theta);
      start_h = -roi_h / 2.0f; start_w = -roi_w / 2.0f;
    } else {
      start_w = roi[1] * a.scale - 0.5f; start_h = roi[2] * a.scale - 0.5f;
      roi_w = roi[3] * a.scale - 0.5f - start_w; roi_h = roi[4] * a.scale - 0.5f - start_h;
    }
    const float bin_h = roi_h / (float)a.PH, bin_w = roi_w / (float)a.PW;
    const int gh = a.sampling_ratio > 0 ? a.sampling_ratio : (int)ceilf(roi_h / (float)a.PH);
    const int gw = a.sampling_ratio > 0 ? a.sampling_ratio : (int)ceilf(roi_w / (float)a.PW);
    const float count = fmaxf((float)(gh * gw), 1.f);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float g[8];
    if (BWD) {
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = dout[i * 8 + e] / count;
    }
    for (int iy = 0; iy < gh; ++iy) {
      const float yy = start_h + ph * bin_h + (iy + 0.5f) * bin_h / (float)gh;
      for (int ix = 0; ix < gw; ++ix) {
        const float xx = start_w + pw * bin_w + (ix + 0.5f) * bin_w / (float)gw;
        float y = yy, x = xx;
        if (a.rotated) { y = yy * cth - xx * sth + ctr_h; x = yy * sth + xx * cth + ctr_w; }
        int yl, xl, yh, xh; float w[4]; bool valid;
        bilinear_setup(y, x, a.H, a.W, yl, xl, yh, xh, w, valid);
        if (!valid) continue;
        const long long base = ((long long)b * a.H) * a.W;
        const long long o00 = ((base + (long long)yl * a.W + xl) * a.C) + c8 * 8, o01 = ((base + (long long)yl * a.W + xh) * a.C) + c8 * 8;
        const long long o10 = ((base + (long long)yh * a.W + xl) * a.C) + c8 * 8, o11 = ((base + (long long)yh * a.W + xh) * a.C) + c8 * 8;
        if (!BWD && XF32) {
          const float* xf = reinterpret_cast<const float*>(a.x);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += w[0] * xf[o00 + e] + w[1] * xf[o01 + e] + w[2] * xf[o10 + e] + w[3] * xf[o11 + e];
        } else if (!BWD) {
          const bf16x8_t v00 = *reinterpret_cast<const bf16x8_t*>(a.x + o00), v01 = *reinterpret_cast<const bf16x8_t*>(a.x + o01);
          const bf16x8_t v10 = *reinterpret_cast<const bf16x8_t*>(a.x + o10), v11 = *reinterpret_cast<const bf16x8_t*>(a.x + o11);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += w[0] * (float)v00[e] + w[1] * (float)v01[e] + w[2] * (float)v10[e] + w[3] * (float)v11[e];
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            atomicAdd(dx + o00 + e, g[e] * w[0]); atomicAdd(dx + o01 + e, g[e] * w[1]);
            atomicAdd(dx + o10 + e, g[e] * w[2]); atomicAdd(dx + o11 + e, g[e] * w[3]);
          }
        }
      }
    }
    if (!BWD) {
#pragma unroll
      for (int e = 0; e < 8; ++e) out[i * 8 + e] = acc[e] / count;
    }
  }
}

// Tiled ROIAlign backward: one workgroup per (roi, 32-channel chunk) accumulates dX for the roi's footprint in 16x16-pixel LDS
// tiles in fixed point (ds_add_u32, see deform_conv.hip for the measurement behind that choice) and flushes each tile with one
// global atomic per touched element, instead of 4 corners x samples x channels global atomics per bin.
// Scale: with max|g| < 2^ex over the (roi, chunk), an addend is v = g * 2^(F - ex) / count * w.  The bilinear weights of one bin's
// samples, divided by the sample count, sum to <= 1, so one bin sends a pixel sum|v| <= 2^F (1 + a few ulp) and the nb = PH * PW
// bins together <= nb * 2^F: the per-pixel sum is bounded by the NUMBER OF BINS (a sub-pixel ROI clamped onto a corner pixel sends
// every bin there), not by a constant.  F = roi_bwd_frac_bits(nb) keeps the sum of the ROUNDED addends inside 31 bits:
//   nb <= 64: F = 24.  sum|rn(v)| <= sum|v| + A / 2 <= 2^30 (1 + a few ulp) + A / 2 for A non-zero addends at the pixel.  A sample
//             reaches a pixel only from its 2x2 support (3x3 with the clamp band of a border pixel); with the adaptive ratio the
//             samples of one axis are > 0.5 px apart (or there is one per bin), with a fixed one A <= 4 nb sr^2 and the entry point
//             keeps sr <= ROI_TILE_MAX_SR: A / 2 < 2^29 either way.
//   nb >  64: F = 29 - ceil(log2 nb).  |rn(v)| <= 2|v| for every v, so sum|rn(v)| <= 2 nb 2^F (1 + a few ulp) <= 2^30 (1 + ...).
// Every addend is rounded to nearest: the error per addend is at most half a step, 2^(ex - F - 1) <= max|g| * 2^-F.
// Output sizes beyond ROI_TILE_MAX_BINS (F would drop below 19 bits) take the generic kernel (sod_roi_align_bwd).
constexpr int ROI_TILE_MAX_BINS = 1024, ROI_TILE_MAX_SR = 1024;
__host__ __device__ inline int roi_bwd_frac_bits(int nb) {
  if (nb <= 64) return 24;
  int lg = 0;
  while ((1 << lg) < nb) ++lg;
  return 29 - lg;
}
constexpr int ROI_T = 16;    // tile edge (pixels)
constexpr int ROI_CC = 32;   // channels per workgroup
__global__ __launch_bounds__(256) void roi_align_bwd_tile_kernel(const RoiArgs a, const float* __restrict__ dout, float* __restrict__ dx) {
  constexpr int PS = ROI_CC + 1, L = ROI_CC / 8;
  __shared__ int win[ROI_T * ROI_T * PS];
  __shared__ float smax[4];
  const int tid = threadIdx.x, r = blockIdx.x, c0 = blockIdx.y * ROI_CC;
  const int cl = tid % L, bl = tid / L, nb = a.PH * a.PW;
  const float* roi = a.rois + (long long)r * (a.rotated ? 6 : 5);
  const int b = (int)roi[0];
  float start_h, start_w, roi_h, roi_w, cth = 1.f, sth = 0.f, ctr_h = 0.f, ctr_w = 0.f;
  float fx0, fx1, fy0, fy1;   // footprint bounds (feature coordinates) of all sample points
  if (a.rotated) {
    ctr_w = roi[1] * a.scale - 0.5f; ctr_h = roi[2] * a.scale - 0.5f;
    roi_w = roi[3] * a.scale; roi_h = roi[4] * a.scale;
    const float theta = roi[5] * 3.14159265358979323846f / 180.0f;
    cth = cosf(theta); sth = sinf(theta);
    start_h = -roi_h / 2.0f; start_w = -roi_w / 2.0f;
    const float ex = 0.5f * (fabsf(roi_w * cth) + fabsf(roi_h * sth)), ey = 0.5f * (fabsf(roi_w * sth) + fabsf(roi_h * cth));
    fx0 = ctr_w - ex; fx1 = ctr_w + ex; fy0 = ctr_h - ey; fy1 = ctr_h + ey;
  } else {
    start_w = roi[1] * a.scale - 0.5f; start_h = roi[2] * a.scale - 0.5f;
    roi_w = roi[3] * a.scale - 0.5f - start_w; roi_h = roi[4] * a.scale - 0.5f - start_h;
    fx0 = fminf(start_w, start_w + roi_w); fx1 = fmaxf(start_w, start_w + roi_w);
    fy0 = fminf(start_h, start_h + roi_h); fy1 = fmaxf(start_h, start_h + roi_h);
  }
  const float bin_h = roi_h / (float)a.PH, bin_w = roi_w / (float)a.PW;
  const int gh = a.sampling_ratio > 0 ? a.sampling_ratio : (int)ceilf(roi_h / (float)a.PH);
  const int gw = a.sampling_ratio > 0 ? a.sampling_ratio : (int)ceilf(roi_w / (float)a.PW);
  const float count = fmaxf((float)(gh * gw), 1.f);
  // pixel window that can receive anything (samples outside [-1, H] x [-1, W] are dropped; the rest clamp into the map)
  const int wx0 = max(0, (int)floorf(fmaxf(fx0, -1.f))), wx1 = min(a.W - 1, (int)floorf(fminf(fx1, (float)a.W)) + 1);
  const int wy0 = max(0, (int)floorf(fmaxf(fy0, -1.f))), wy1 = min(a.H - 1, (int)floorf(fminf(fy1, (float)a.H)) + 1);
  if (wx1 < wx0 || wy1 < wy0 || gh <= 0 || gw <= 0) return;
  // fixed-point scale from max |g| of this (roi, chunk)
  float gmax = 0.f;
  for (int bin = bl; bin < nb; bin += 256 / L) {
    const float* gp = dout + ((long long)r * nb + bin) * a.C + c0 + cl * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) gmax = fmaxf(gmax, fabsf(gp[e]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, o, 64));
  if ((tid & 63) == 0) smax[tid >> 6] = gmax;
  __syncthreads();
  gmax = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  if (gmax == 0.f || !(gmax < 3.0e38f)) return;   // nothing to add / non-finite gradient (the loss is already non-finite then)
  int ex = 0;
  (void)frexpf(gmax, &ex);
  const int F = roi_bwd_frac_bits(nb);
  const float S = ldexpf(1.f, F - ex) / count, invS = ldexpf(1.f, ex - F);
  const long long base = ((long long)b * a.H) * a.W;
  for (int ty = wy0; ty <= wy1; ty += ROI_T)
    for (int tx = wx0; tx <= wx1; tx += ROI_T) {
      for (int i = tid; i < ROI_T * ROI_T * PS; i += 256) win[i] = 0;
      __syncthreads();
      // work item = one ROW of a bin's sample grid (bin, iy), dealt out over the 256 / L lane groups.  A row whose bounding box (+2 px: the
      // bilinear neighbour and the clamp into the map) misses this tile is skipped before anything is loaded: with the adaptive sampling
      // ratio (ceil(roi / 7) samples per bin side) a large ROI has ~1 sample per feature pixel, and visiting every sample for every
      // 16x16 tile of its footprint made the work quadratic in the ROI's area (3.4 ms per step for the rotated R-CNN's 8192 ROIs).
      for (int item = bl; item < nb * gh; item += 256 / L) {
        const int bin = item / gh, iy = item - bin * gh;
        const int ph = bin / a.PW, pw = bin - ph * a.PW;
        const float yy = start_h + ph * bin_h + (iy + 0.5f) * bin_h / (float)gh;
        {
          const float xa = start_w + pw * bin_w + 0.5f * bin_w / (float)gw, xb = start_w + pw * bin_w + ((float)gw - 0.5f) * bin_w / (float)gw;
          float ya0 = yy, xa0 = xa, yb0 = yy, xb0 = xb;
          if (a.rotated) { ya0 = yy * cth - xa * sth + ctr_h; xa0 = yy * sth + xa * cth + ctr_w; yb0 = yy * cth - xb * sth + ctr_h; xb0 = yy * sth + xb * cth + ctr_w; }
          if (fmaxf(xa0, xb0) + 2.f < (float)tx || fminf(xa0, xb0) - 2.f > (float)(tx + ROI_T - 1) ||
              fmaxf(ya0, yb0) + 2.f < (float)ty || fminf(ya0, yb0) - 2.f > (float)(ty + ROI_T - 1)) continue;
        }
        const float* gp = dout + ((long long)r * nb + bin) * a.C + c0 + cl * 8;
        float g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = gp[e] * S;
        {
          for (int ix = 0; ix < gw; ++ix) {
            const float xx = start_w + pw * bin_w + (ix + 0.5f) * bin_w / (float)gw;
            float y = yy, x = xx;
            if (a.rotated) { y = yy * cth - xx * sth + ctr_h; x = yy * sth + xx * cth + ctr_w; }
            int yl, xl, yh, xh; float w[4]; bool valid;
            bilinear_setup(y, x, a.H, a.W, yl, xl, yh, xh, w, valid);
            if (!valid) continue;
            const int ys[2] = {yl - ty, yh - ty}, xs[2] = {xl - tx, xh - tx};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int py = ys[k >> 1], px = xs[k & 1];
              if (py < 0 || py >= ROI_T || px < 0 || px >= ROI_T) continue;
              int* wp = win + (py * ROI_T + px) * PS + cl * 8;
#pragma unroll
              for (int e = 0; e < 8; ++e) atomicAdd(wp + e, __float2int_rn(g[e] * w[k]));
            }
          }
        }
      }
      __syncthreads();
      for (int i = tid; i < ROI_T * ROI_T * ROI_CC; i += 256) {
        const int c = i % ROI_CC, p = i / ROI_CC;
        const int q = win[p * PS + c];
        if (q != 0) {
          const int py = ty + p / ROI_T, px = tx + p % ROI_T;
          atomicAdd(dx + ((base + (long long)py * a.W + px) * a.C) + c0 + c, (float)q * invS);
        }
      }
      __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- box losses on XYXY
// the pair policies of pair_loss.h.  fvcore giou_loss (eps 1e-7): per-row loss and gradient w.r.t. boxes1
struct GiouXyxyPair {
  static constexpr int W = 4;
  using Lds = void;
  static constexpr int LDS_PER_LANE = 0;
  static __device__ __forceinline__ float pair(const float* a, const float* b, float eps, void*, bool want_grad, float* g) {
    return giou_pair(a, b, eps, want_grad ? g : nullptr);
  }
};

// fvcore smooth_l1_loss, one element a pair; beta < 1e-5: plain L1
struct SmoothL1Pair {
  static constexpr int W = 1;
  using Lds = void;
  static constexpr int LDS_PER_LANE = 0;
  static __device__ __forceinline__ float pair(const float* x, const float* t, float beta, void*, bool want_grad, float* g) {
    const float d = x[0] - t[0], ad = fabsf(d);
    float l, gd;
    if (beta < 1e-5f) { l = ad; gd = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
    else if (ad < beta) { l = 0.5f * d * d / beta; gd = d / beta; }
    else { l = ad - 0.5f * beta; gd = d > 0.f ? 1.f : -1.f; }
    if (want_grad) g[0] = gd;
    return l;
  }
};

// ---------------------------------------------------------------------------------------------- anchor labelling
// Matcher(thresholds=[lo,hi], labels=[l0,l1,l2], allow_low_quality_matches) over pairwise_iou(gt (G), anchors (A)) without the
// G x A matrix: pass 1 = per-anchor max/argmax over gts + per-gt max over anchors (atomicMax on float bits, IoU >= 0);
// pass 2 = thresholds + low-quality promotion (anchor ties with the per-gt best, as `Q == best_per_gt[:, None]`).
// (pair_iou, the XYXY IoU of pairwise_iou, lives in common.h: the batched matcher of fcos_rpd.hip must reproduce it bit for bit)

// D = 4: XYXY boxes (pairwise_iou); D = 5: (cx, cy, w, h, angle) boxes (pairwise_iou_rotated, RRPN / RROIHeads)
template <int D>
__device__ __forceinline__ float match_iou(const float* g, const float* a) {
  if (D == 4) return pair_iou(g, a);
  return fmaxf(iou_rotated(g, a), 0.f);
}

template <int D>
__global__ __launch_bounds__(256) void anchor_match1_kernel(const float* __restrict__ gts, int G, const float* __restrict__ anchors, int A,
                                                            float* __restrict__ best_val, int* __restrict__ best_idx,
                                                            unsigned* __restrict__ gt_best_bits) {
  extern __shared__ unsigned lbest[];   // [G]
  __shared__ P2 rot_pts[D == 5 ? 24 * 256 : 1];
  for (int g = threadIdx.x; g < G; g += 256) lbest[g] = 0u;
  __syncthreads();
  for (int i = blockIdx.x * 256 + threadIdx.x; i < A; i += gridDim.x * 256) {
    float a[D];
#pragma unroll
    for (int e = 0; e < D; ++e) a[e] = anchors[(long long)i * D + e];
    float bv = -1.f; int bi = 0;
    for (int g = 0; g < G; ++g) {
      float v;
      if constexpr (D == 5) v = fmaxf(iou_rotated_lds(gts + g * D, a, rot_pts + threadIdx.x, 256), 0.f);
      else v = match_iou<D>(gts + g * D, a);
      if (v > bv) { bv = v; bi = g; }            // first maximum wins (torch.max(dim=0))
      if (v > 0.f) atomicMax(&lbest[g], __float_as_uint(v));  // v >= 0: uint order == float order; lbest starts at 0, so a zero changes nothing
                                                             // (and almost every pair is a zero: 256 threads on one LDS word serialise)
    }
    best_val[i] = bv; best_idx[i] = bi;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) atomicMax(&gt_best_bits[g], lbest[g]);
}

// Rotated boxes: anchor_match1_kernel<5> above pays the polygon clipping per WAVE for every box some lane is near (64 consecutive anchors =
// 3.5 locations x 18 shapes: near a box that is every wave, 150 of its 200 us for the 1.6 M RRPN anchors).  This variant tests all (anchor,
// box) pairs of a 256-anchor chunk with the circle test only, compacts the survivors through LDS and deals them out evenly over the
// threads; per-anchor maximum with "first maximum wins" = 64-bit LDS atomicMax of (IoU bits, ~box index).  Same values, same argmax.
__global__ __launch_bounds__(256) void anchor_match1_rot_kernel(const float* __restrict__ gts, int G, const float* __restrict__ anchors, int A,
                                                                float* __restrict__ best_val, int* __restrict__ best_idx,
                                                                unsigned* __restrict__ gt_best_bits) {
  extern __shared__ unsigned lbest[];   // [G]
  constexpr int GS = 8;                 // boxes per round: at most 256 * GS pairs
  __shared__ unsigned pairs[256 * GS];
  __shared__ P2 rot_pts[24 * 256];      // 48 KB: the clipping's candidate points (see RotPtsLds)
  __shared__ unsigned long long abest[256];
  __shared__ int npairs;
  const int tid = threadIdx.x;
  for (int g = tid; g < G; g += 256) lbest[g] = 0u;
  const int chunks = (A + 255) / 256;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int i = ch * 256 + tid;
    float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < A) {
#pragma unroll
      for (int e = 0; e < 5; ++e) a[e] = anchors[(long long)i * 5 + e];
    }
    const float ra = 0.5f * sqrtf(a[2] * a[2] + a[3] * a[3]);
    const bool live = i < A && a[2] * a[3] >= 1e-14f;
    abest[tid] = 0x00000000FFFFFFFFull;          // IoU 0 with box 0: what "v > bv" from bv = -1 leaves when every IoU is 0
    for (int g0 = 0; g0 < G; g0 += GS) {
      if (tid == 0) npairs = 0;
      __syncthreads();
      if (live) {
        const int g1 = min(G, g0 + GS);
        for (int g = g0; g < g1; ++g) {
          const float* b = gts + g * 5;
          // the two early returns of iou_rotated: a pair dropped here has IoU exactly 0 there
          const float dx = b[0] - a[0], dy = b[1] - a[1], rs = ra + 0.5f * sqrtf(b[2] * b[2] + b[3] * b[3]);
          if (b[2] * b[3] >= 1e-14f && dx * dx + dy * dy <= rs * rs * 1.0001f) pairs[atomicAdd(&npairs, 1)] = ((unsigned)tid << 16) | (unsigned)(g - g0);
        }
      }
      __syncthreads();
      const int np = npairs;
      for (int t = tid; t < np; t += 256) {
        const unsigned pr = pairs[t];
        const int la = (int)(pr >> 16), g = g0 + (int)(pr & 0xffffu);
        float aa[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) aa[e] = anchors[((long long)ch * 256 + la) * 5 + e];
        const float v = fmaxf(iou_rotated_lds(gts + g * 5, aa, rot_pts + tid, 256), 0.f);
        if (v > 0.f) {
          atomicMax(&abest[la], ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)g));
          atomicMax(&lbest[g], __float_as_uint(v));
        }
      }
      __syncthreads();
    }
    if (i < A) {
      const unsigned long long bb = abest[tid];
      best_val[i] = __uint_as_float((unsigned)(bb >> 32));
      best_idx[i] = (int)(0xFFFFFFFFu - (unsigned)(bb & 0xFFFFFFFFull));
    }
    __syncthreads();
  }
  __syncthreads();
  for (int g = tid; g < G; g += 256) atomicMax(&gt_best_bits[g], lbest[g]);
}

template <int D>
__global__ __launch_bounds__(256) void anchor_match2_kernel(const float* __restrict__ gts, int G, const float* __restrict__ anchors, int A,
                                                            const float* __restrict__ best_val, const unsigned* __restrict__ gt_best_bits,
                                                            float lo, float hi, int l0, int l1, int l2, int low_quality,
                                                            signed char* __restrict__ labels) {
  __shared__ P2 rot_pts[D == 5 ? 24 * 256 : 1];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < A; i += gridDim.x * 256) {
    const float v = best_val[i];
    int lab = (v < lo) ? l0 : ((v < hi) ? l1 : l2);
    if (low_quality) {
      float a[D];
#pragma unroll
      for (int e = 0; e < D; ++e) a[e] = anchors[(long long)i * D + e];
      for (int g = 0; g < G; ++g) {
        float v;
        if constexpr (D == 5) v = fmaxf(iou_rotated_lds(gts + g * D, a, rot_pts + threadIdx.x, 256), 0.f);
        else v = match_iou<D>(gts + g * D, a);
        if (v == __uint_as_float(gt_best_bits[g])) { lab = 1; break; }
      }
    }
    labels[i] = (signed char)lab;
  }
}

// ---------------------------------------------------------------------------------------------- RetinaNet targets (the box loss: retina_box_loss.hip)
// label_anchors tail (retina_rotated.py:279-291) + Box2BoxTransform.get_deltas for one image
__global__ __launch_bounds__(256) void retina_targets_kernel(const float* __restrict__ anchors, int A, const float* __restrict__ gts,
                                                             const int* __restrict__ gt_classes, int G, const int* __restrict__ matches,
                                                             const signed char* __restrict__ mlabels, int num_classes, float wx, float wy,
                                                             float ww, float wh, int* __restrict__ gt_labels, float* __restrict__ deltas) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < A; i += gridDim.x * 256) {
    int lab = num_classes;
    f32x4_t d = {0.f, 0.f, 0.f, 0.f};
    if (G > 0) {
      const int m = matches[i];
      const int ml = mlabels[i];
      lab = (ml == 0) ? num_classes : ((ml == -1) ? -1 : gt_classes[m]);
      const f32x4_t s = *reinterpret_cast<const f32x4_t*>(anchors + (long long)i * 4);
      const f32x4_t t = *reinterpret_cast<const f32x4_t*>(gts + (long long)m * 4);
      const float w[4] = {wx, wy, ww, wh};
      float o[4];
      xyxy_get_deltas(s, t, w, o);
      d = f32x4_t{o[0], o[1], o[2], o[3]};
    }
    gt_labels[i] = lab;
    *reinterpret_cast<f32x4_t*>(deltas + (long long)i * 4) = d;
  }
}

}  // namespace

extern "C" int sod_box_iou_rotated(const float* boxes1, int n1, const float* boxes2, int n2, float* iou_out, void* stream) {
  if (n1 < 0 || n2 < 0 || ((long long)n1 * n2 > 0 && (!boxes1 || !boxes2 || !iou_out))) return SOD_EARG;
  if ((long long)n1 * n2 == 0) return SOD_OK;
  SOD_LAUNCH(pairwise_iou_rotated_kernel, dim3(sod_nblk((long long)n1 * n2, 4096)), dim3(256), 0, (hipStream_t)stream, boxes1, n1, boxes2, n2, iou_out);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

static int roi_fill(RoiArgs& a, const void* x, const float* rois, int R, int N, int H, int W, int C, int PH, int PW, float scale,
                    int sampling_ratio, int rotated) {
  if (!x || (!rois && R > 0) || R < 0 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || PH <= 0 || PW <= 0) return SOD_EARG;
  a.x = (const __bf16*)x; a.rois = rois; a.R = R; a.N = N; a.H = H; a.W = W; a.C = C; a.PH = PH; a.PW = PW;
  a.scale = scale; a.sampling_ratio = sampling_ratio; a.rotated = rotated;
  return SOD_OK;
}

extern "C" int sod_roi_align_fwd(const void* x, const float* rois, float* out, int R, int N, int H, int W, int C, int PH, int PW,
                                 float spatial_scale, int sampling_ratio, int rotated, void* stream) {
  RoiArgs a{};
  int rc = roi_fill(a, x, rois, R, N, H, W, C, PH, PW, spatial_scale, sampling_ratio, rotated);
  if (rc) return rc;
  if (R == 0) return SOD_OK;      // nothing to do: rois and out of an empty call may be NULL
  if (!out) return SOD_EARG;
  SOD_LAUNCH((roi_align_kernel<false, false>), dim3(sod_nblk((long long)R * PH * PW * (C / 8), 8192)), dim3(256), 0, (hipStream_t)stream, a, out, nullptr, nullptr);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_roi_align_fwd_f32(const float* x, const float* rois, float* out, int R, int N, int H, int W, int C, int PH, int PW,
                                     float spatial_scale, int sampling_ratio, int rotated, void* stream) {
  RoiArgs a{};
  int rc = roi_fill(a, x, rois, R, N, H, W, C, PH, PW, spatial_scale, sampling_ratio, rotated);
  if (rc) return rc;
  if (R == 0) return SOD_OK;      // nothing to do: rois and out of an empty call may be NULL
  if (!out) return SOD_EARG;
  SOD_LAUNCH((roi_align_kernel<false, true>), dim3(sod_nblk((long long)R * PH * PW * (C / 8), 8192)), dim3(256), 0, (hipStream_t)stream, a, out, nullptr, nullptr);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_roi_align_bwd(const float* dout, const float* rois, float* dx, int R, int N, int H, int W, int C, int PH, int PW,
                                 float spatial_scale, int sampling_ratio, int rotated, void* stream) {
  RoiArgs a{};
  int rc = roi_fill(a, dx, rois, R, N, H, W, C, PH, PW, spatial_scale, sampling_ratio, rotated);   // x unused in bwd
  if (rc) return rc;
  if (R == 0) return SOD_OK;
  if (!dout) return SOD_EARG;
  // the tiles' fixed point is proven for these output sizes and sampling ratios only (see roi_align_bwd_tile_kernel)
  if (C % ROI_CC == 0 && C / ROI_CC <= 65535 && (long long)PH * PW <= ROI_TILE_MAX_BINS && sampling_ratio <= ROI_TILE_MAX_SR) {
    SOD_LAUNCH(roi_align_bwd_tile_kernel, dim3(R, C / ROI_CC), dim3(256), 0, (hipStream_t)stream, a, dout, dx);
    SOD_CHECK_LAUNCH();
    return SOD_OK;
  }
  SOD_LAUNCH((roi_align_kernel<true, false>), dim3(sod_nblk((long long)R * PH * PW * (C / 8), 8192)), dim3(256), 0, (hipStream_t)stream, a, nullptr, dout, dx);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_giou_loss_xyxy(const float* boxes1, const float* boxes2, long long P, float eps, float* elem_out, float* sum_out,
                                  const float* grad_scale, float* dboxes1, float* ws, void* stream) {
  return launch_pairs<GiouXyxyPair>(boxes1, boxes2, P, eps, elem_out, sum_out, grad_scale, dboxes1, ws, stream);
}

extern "C" int sod_smooth_l1_loss(const float* input, const float* target, long long n, float beta, float* elem_out, float* sum_out,
                                  const float* grad_scale, float* dinput, float* ws, void* stream) {
  return launch_pairs<SmoothL1Pair>(input, target, n, beta, elem_out, sum_out, grad_scale, dinput, ws, stream);
}

template <int D>
static int anchor_match_impl(const float* gt_boxes, int G, const float* anchors, int A, float thr_lo, float thr_hi,
                             int label_below, int label_between, int label_above, int allow_low_quality,
                             float* matched_vals, int* matches, signed char* labels, unsigned* gt_best_ws, void* stream) {
  if (!anchors || A <= 0 || !matched_vals || !matches || !labels || G < 0 || G > 4096) return SOD_EARG;
  hipStream_t st = (hipStream_t)stream;
  if (G == 0) {   // Matcher on an empty gt set: everything unmatched with the lowest label
    hipError_t e = hipMemsetAsync(matches, 0, sizeof(int) * A, st);
    if (e == hipSuccess) e = hipMemsetAsync(matched_vals, 0, sizeof(float) * A, st);
    if (e == hipSuccess) e = hipMemsetAsync(labels, label_below & 0xff, A, st);
    return (int)e;
  }
  if (!gt_boxes || !gt_best_ws) return SOD_EARG;
  hipError_t e = hipMemsetAsync(gt_best_ws, 0, sizeof(unsigned) * G, st);
  if (e != hipSuccess) return (int)e;
  const int g = sod_nblk(A, 2048);
  if (D == 5) SOD_LAUNCH(anchor_match1_rot_kernel, dim3(g), dim3(256), sizeof(unsigned) * G, st, gt_boxes, G, anchors, A, matched_vals, matches, gt_best_ws);
  else SOD_LAUNCH(anchor_match1_kernel<D>, dim3(g), dim3(256), sizeof(unsigned) * G, st, gt_boxes, G, anchors, A, matched_vals, matches, gt_best_ws);
  SOD_LAUNCH(anchor_match2_kernel<D>, dim3(g), dim3(256), 0, st, gt_boxes, G, anchors, A, matched_vals, gt_best_ws, thr_lo, thr_hi,
             label_below, label_between, label_above, allow_low_quality, labels);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

// ROIHeads.label_and_sample_proposals' matching + labelling for the WHOLE batch in one launch: proposal r of image n (rows >= counts[n] are
// padding) against that image's boxes gt[gt_off[n] .. gt_off[n + 1]): best IoU with "first maximum wins", Matcher([thr], [l0, l1]) without
// low-quality matches, class = the matched box's class for label 1, num_classes for label 0, -1 for label -1 and for padding rows.
template <int D>
__global__ __launch_bounds__(256) void roi_label_batched_kernel(const float* __restrict__ boxes, const int* __restrict__ counts, int R,
                                                                const float* __restrict__ gt, const int* __restrict__ gt_classes,
                                                                const int* __restrict__ gt_off, float thr, int l0, int l1, int num_classes,
                                                                int* __restrict__ matches, signed char* __restrict__ cls) {
  __shared__ P2 rot_pts[D == 5 ? 24 * 256 : 1];
  const int n = blockIdx.y;
  const int g0 = gt_off[n], G = gt_off[n + 1] - g0, cnt = counts[n];
  for (int r = blockIdx.x * 256 + threadIdx.x; r < R; r += gridDim.x * 256) {
    const long long o = (long long)n * R + r;
    if (r >= cnt) { matches[o] = 0; cls[o] = -1; continue; }
    float a[D];
#pragma unroll
    for (int e = 0; e < D; ++e) a[e] = boxes[o * D + e];
    float bv = -1.f; int bi = 0;
    for (int g = 0; g < G; ++g) {
      float v;
      if constexpr (D == 5) v = fmaxf(iou_rotated_lds(gt + (long long)(g0 + g) * D, a, rot_pts + threadIdx.x, 256), 0.f);
      else v = match_iou<D>(gt + (long long)(g0 + g) * D, a);
      if (v > bv) { bv = v; bi = g; }
    }
    int c = num_classes;                            // no boxes: everything is background (matches stay 0)
    if (G > 0) {
      const int lab = (bv < thr) ? l0 : l1;
      c = (lab == 0) ? num_classes : ((lab == -1) ? -1 : gt_classes[g0 + bi]);
    }
    matches[o] = bi;
    cls[o] = (signed char)c;
  }
}

extern "C" int sod_roi_label_batched(const float* boxes, const int* counts, int N, int R, int box_dim, const float* gt_boxes, const int* gt_classes,
                                     const int* gt_off, float iou_threshold, int label_below, int label_above, int num_classes, int* matches,
                                     signed char* classes, void* stream) {
  if (!boxes || !counts || !gt_off || !matches || !classes || N <= 0 || N > 65535 || R <= 0 || (box_dim != 4 && box_dim != 5) || num_classes <= 0 ||
      num_classes > 126)
    return SOD_EARG;
  const dim3 grid((R + 255) / 256, N);
  if (box_dim == 4) SOD_LAUNCH(roi_label_batched_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, boxes, counts, R, gt_boxes, gt_classes, gt_off,
                               iou_threshold, label_below, label_above, num_classes, matches, classes);
  else SOD_LAUNCH(roi_label_batched_kernel<5>, grid, dim3(256), 0, (hipStream_t)stream, boxes, counts, R, gt_boxes, gt_classes, gt_off, iou_threshold,
                  label_below, label_above, num_classes, matches, classes);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_anchor_match(const float* gt_boxes, int G, const float* anchors, int A, float thr_lo, float thr_hi,
                                int label_below, int label_between, int label_above, int allow_low_quality,
                                float* matched_vals, int* matches, signed char* labels, unsigned* gt_best_ws, void* stream) {
  return anchor_match_impl<4>(gt_boxes, G, anchors, A, thr_lo, thr_hi, label_below, label_between, label_above, allow_low_quality, matched_vals,
                              matches, labels, gt_best_ws, stream);
}

extern "C" int sod_anchor_match_rotated(const float* gt_boxes, int G, const float* anchors, int A, float thr_lo, float thr_hi,
                                        int label_below, int label_between, int label_above, int allow_low_quality,
                                        float* matched_vals, int* matches, signed char* labels, unsigned* gt_best_ws, void* stream) {
  return anchor_match_impl<5>(gt_boxes, G, anchors, A, thr_lo, thr_hi, label_below, label_between, label_above, allow_low_quality, matched_vals,
                              matches, labels, gt_best_ws, stream);
}

extern "C" int sod_retina_targets(const float* anchors, int A, const float* gt_boxes, const int* gt_classes, int G, const int* matches,
                                  const signed char* match_labels, int num_classes, const float* weights4, int* gt_labels, float* gt_deltas,
                                  void* stream) {
  if (!anchors || A <= 0 || !gt_labels || !gt_deltas || !weights4 || (G > 0 && (!gt_boxes || !gt_classes || !matches || !match_labels))) return SOD_EARG;
  SOD_LAUNCH(retina_targets_kernel, dim3(sod_nblk(A, 2048)), dim3(256), 0, (hipStream_t)stream, anchors, A, gt_boxes, gt_classes, G, matches, match_labels,
             num_classes, weights4[0], weights4[1], weights4[2], weights4[3], gt_labels, gt_deltas);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
