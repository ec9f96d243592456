// COCO box evaluation for rotated boxes (cx, cy, w, h, angle_deg) on device: the per-(image, category) greedy matching of
// detectron2's RotatedCOCOeval.computeIoU (pairwise_iou_rotated, float32) under pycocotools' COCOeval.evaluateImg
// (call site train_net.py:60-62, evaluator type "rotated_coco").  The accumulation is sod_coco_accumulate (coco_eval.hip), unchanged.
// The slenderness-bucketed recall pass (AR / mAR) on rotated boxes is the skeleton of proposal_ar.h under the box policy ArRotBox.
//
// The IoU is iou_rotated_impl of rotated_iou.h with the candidate points in LDS - the function box_iou_rotated and the rotated NMS
// run, so a threshold decides here on the same float32 bits as there.
#include "common.h"
#include "../../include/slender_hip.h"

namespace {

#include "rotated_iou.h"

constexpr int ROT_MAX_T = 16;
constexpr int ROT_MAX_A = 8;
constexpr int ROT_LDS_IOU = 3200;      // floats of the staged [D, G] IoU matrix of one segment (12.8 KB); larger segments use scratch

struct RotMatchParams {
  double iou_thr[ROT_MAX_T];
  double lo[ROT_MAX_A], hi[ROT_MAX_A];
};

// floats of the IoU part of a segment's scratch slot: even, so that the 8-byte "taken" rows behind it stay aligned
__host__ __device__ inline long long rot_iou_slot(int num_gts, int max_det) { return ((long long)max_det * num_gts + 1) & ~1LL; }

// One workgroup (one wave) per (category k, image i) segment s = k * num_img + i.  All 64 lanes stage the [D, G] IoU matrix; then lane
// t * A + a runs the greedy scan of evaluateImg for IoU threshold t and value range a; the per-detection results of all lanes are one
// ballot each.  The range test is generic: gt_val / dt_val are areas for COCO's area ranges, ratios for the slenderness ranges.
__global__ __launch_bounds__(64) void coco_match_rotated_kernel(const int* __restrict__ gt_off, const float* __restrict__ gt_box,
                                                                const unsigned char* __restrict__ gt_crowd, const double* __restrict__ gt_val,
                                                                const int* __restrict__ dt_off, const float* __restrict__ dt_box,
                                                                const double* __restrict__ dt_val, int num_img, int max_det, int T, int A,
                                                                RotMatchParams p, const long long* __restrict__ scratch_off,
                                                                float* __restrict__ scratch, unsigned long long* __restrict__ dt_matched,
                                                                unsigned long long* __restrict__ dt_ignored, int* __restrict__ npig) {
  __shared__ float s_iou[ROT_LDS_IOU];
  __shared__ P2 rot_pts[24 * 64];      // 12 KB: the clipping's candidate points (see RotPtsLds)
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  const int g0 = gt_off[s], G = gt_off[s + 1] - g0;
  const int d0 = dt_off[s];
  const int D = min(dt_off[s + 1] - d0, max_det);
  if (G == 0 && D == 0) return;   // evaluateImg returns None: the segment takes no part in accumulate
  const int k = s / num_img;
  const bool active = lane < T * A;
  const int t = active ? lane / A : 0, a = active ? lane % A : 0;
  const double lo = p.lo[a], hi = p.hi[a];
  if (lane < A) {
    int c = 0;
    for (int g = 0; g < G; ++g) {
      const double r = gt_val[g0 + g];
      c += !(gt_crowd[g0 + g] || r < p.lo[lane] || r > p.hi[lane]);
    }
    if (c) atomicAdd(npig + k * A + lane, c);
  }
  if (D == 0) return;
  // IoUs [D, G] (detection first, gt second) staged once for all lanes: LDS, or this segment's slot of the global scratch
  const bool in_lds = (long long)D * G <= ROT_LDS_IOU;
  float* iou = in_lds ? s_iou : scratch + scratch_off[s];
  for (int idx = lane; idx < D * G; idx += 64) {
    const int d = idx / G, g = idx - d * G;
    iou[idx] = iou_rotated_lds(dt_box + 5 * (size_t)(d0 + d), gt_box + 5 * (size_t)(g0 + g), rot_pts + lane, 64);
  }
  __syncthreads();
  // matched-gt flags of this lane: one register word for G <= 64, else a bit row in the scratch slot after the IoUs
  unsigned long long taken0 = 0;
  unsigned long long* taken = nullptr;
  const int words = (G + 63) / 64;
  if (G > 64) {
    taken = (unsigned long long*)(scratch + scratch_off[s] + rot_iou_slot(G, max_det)) + (size_t)lane * words;
    if (active)
      for (int w = 0; w < words; ++w) taken[w] = 0ull;
  }
  // torch compares a float32 IoU with the float64 threshold in float32
  const float thr = (float)fmin(p.iou_thr[t], 1.0 - 1e-10);
  for (int d = 0; d < D; ++d) {
    bool mt = false, ig = false;
    if (active) {
      float best = thr;
      int m = -1;
      bool m_ig = false;
      // the gts in stable order with the ignored ones last: the non-ignored pass, then (unless a real gt matched) the ignored pass
      for (int pass = 0; pass < 2 && !(m >= 0 && !m_ig); ++pass) {
        for (int g = 0; g < G; ++g) {
          const double r = gt_val[g0 + g];
          const bool crowd = gt_crowd[g0 + g] != 0;
          const bool gig = crowd || r < lo || r > hi;
          if (gig != (pass == 1)) continue;
          const bool tk = G > 64 ? ((taken[g >> 6] >> (g & 63)) & 1ull) : ((taken0 >> g) & 1ull);
          if (tk && !crowd) continue;
          const float v = iou[(size_t)d * G + g];
          if (v < best) continue;
          best = v;
          m = g;
          m_ig = gig;
        }
      }
      if (m >= 0) {
        mt = true;
        ig = m_ig;
        if (G > 64) taken[m >> 6] |= 1ull << (m & 63);
        else taken0 |= 1ull << m;
      } else {
        const double v = dt_val[d0 + d];
        ig = v < lo || v > hi;
      }
    }
    const unsigned long long bm = __ballot(mt), bi = __ballot(ig);
    if (lane == 0) {
      dt_matched[d0 + d] = bm;
      dt_ignored[d0 + d] = bi;
    }
  }
}

#include "proposal_ar.h"

// The recall pass on rotated boxes.  Two of the four waves stage the matrices: 24 candidate points x 128 lanes x 8 B = 24 KB of LDS beside
// the two staged matrices (25.6 KB) and the reduction arrays (6 KB) - 55.6 KB of the 64 KB a workgroup may declare; with all 256 lanes the
// points alone would take 48 KB.  The rounds run on all four waves.  A gt's area bucket is decided by the float32 product w * h.
struct ArRotBox {
  static constexpr int W = 5;
  static constexpr int STAGE_LANES = 128;
  using Lds = P2;
  static constexpr int LDS_PER_LANE = 24;
  static __device__ __forceinline__ float overlap(const float* d, const float* g, Lds* lds) {
    return iou_rotated_lds(d, g, lds, STAGE_LANES);
  }
  static __device__ __forceinline__ float area(const float* g) { return g[2] * g[3]; }
};

}  // namespace

extern "C" long long sod_proposal_ar_rotated_scratch_floats(int num_gts, int limit) { return proposal_ar_scratch_floats(num_gts, limit); }

extern "C" int sod_proposal_ar_rotated(const int* gt_off, const float* gt_box5, const int* gt_cls, const float* gt_ratio, const int* dt_off,
                                       const long long* dt_order, const float* dt_box5, const int* dt_cls, int num_img, int limit, int K1,
                                       const float* thr, int T, const float* ratio_rng, int R, const float* area_rng, int A,
                                       const long long* scratch_off, float* scratch, int* hits, int* counts, float* recalls,
                                       void* stream) {
  return launch_proposal_ar<ArRotBox>(gt_off, gt_box5, gt_cls, gt_ratio, dt_off, dt_order, dt_box5, dt_cls, num_img, limit, K1, thr, T,
                                      ratio_rng, R, area_rng, A, scratch_off, scratch, hits, counts, recalls, stream);
}

extern "C" long long sod_coco_match_rotated_scratch_floats(int num_gts, int max_det) {
  if (num_gts < 0 || max_det < 0) return -1;
  if ((long long)num_gts * max_det <= ROT_LDS_IOU && num_gts <= 64) return 0;
  return rot_iou_slot(num_gts, max_det) + (num_gts > 64 ? 2LL * 64 * ((num_gts + 63) / 64) : 0);
}

extern "C" int sod_coco_match_rotated(const int* gt_off, const float* gt_box5, const unsigned char* gt_crowd, const double* gt_val,
                                      const int* dt_off, const float* dt_box5, const double* dt_val, int num_seg, int num_img,
                                      int max_det, const double* iou_thr, int T, const double* ranges, int A,
                                      const long long* scratch_off, float* scratch, unsigned long long* dt_matched,
                                      unsigned long long* dt_ignored, int* npig, void* stream) {
  if (num_seg < 0 || num_img <= 0 || num_seg % num_img || max_det <= 0 || T <= 0 || A <= 0 || T > ROT_MAX_T || A > ROT_MAX_A ||
      T * A > 64 || !iou_thr || !ranges || !gt_off || !dt_off || !scratch_off || !npig)
    return SOD_EARG;
  if (num_seg == 0) return SOD_OK;
  RotMatchParams p;
  for (int t = 0; t < T; ++t) p.iou_thr[t] = iou_thr[t];
  for (int a = 0; a < A; ++a) {
    p.lo[a] = ranges[2 * a];
    p.hi[a] = ranges[2 * a + 1];
  }
  SOD_LAUNCH(coco_match_rotated_kernel, dim3(num_seg), dim3(64), 0, (hipStream_t)stream, gt_off, gt_box5, gt_crowd, gt_val, dt_off,
             dt_box5, dt_val, num_img, max_det, T, A, p, scratch_off, scratch, dt_matched, dt_ignored, npig);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
