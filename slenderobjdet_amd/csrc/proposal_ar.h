// The skeleton of the slenderness-bucketed recall pass (_evaluate_predictions_ar, coco_evaluation.py:283-417): ONE kernel template holds
// the greedy "best covered gt, first box that covers it best" rounds - one workgroup per image, the class-agnostic and the class-masked
// [D, G] overlap matrices staged in LDS or in the image's scratch slot, min(D, G) rounds, integer atomics - and a box policy supplies what
// depends on the box form:
//   ArXywhBox   sod_proposal_ar           coco_eval.hip           W = 4, XYWH, detectron2's pairwise_iou rebuilt in float32
//   ArRotBox    sod_proposal_ar_rotated   coco_eval_rotated.hip   W = 5, (cx, cy, w, h, angle_deg), iou_rotated_lds of rotated_iou.h
// A policy has: W (floats per box); STAGE_LANES (the first STAGE_LANES threads of the workgroup fill the matrices: whole waves, at most
// AR_THREADS); Lds and LDS_PER_LANE (element type and per-lane count of an LDS array the kernel owns for the overlap, lane stride
// STAGE_LANES; void and 0: none); overlap(dt, gt, lds) -> float32 and area(gt) -> the float32 area that decides the gt's area bucket.
// The including file places this header inside its own anonymous namespace, after common.h (and after rotated_iou.h where its policy
// needs it).
#pragma once

constexpr int AR_LDS_IOU = 3200;      // floats per staged [D, G] matrix of one image (two matrices: 25.6 KB)
constexpr int AR_THREADS = 256;
constexpr int AR_MAX_T = 16;
constexpr int AR_MAX_A = 8;

struct ArParams {
  float thr[AR_MAX_T];
  float rlo[AR_MAX_A], rhi[AR_MAX_A];
  float alo[AR_MAX_A], ahi[AR_MAX_A];
};

// bit r of the ratio ranges / bit 8 + a of the area ranges a gt falls in (inclusive bounds, float32)
__device__ __forceinline__ int ar_buckets(float area, float ratio, const ArParams& p, int R, int A) {
  int bits = 0;
  for (int r = 0; r < R; ++r) bits |= (ratio >= p.rlo[r] && ratio <= p.rhi[r]) << r;
  for (int a = 0; a < A; ++a) bits |= (area >= p.alo[a] && area <= p.ahi[a]) << (8 + a);
  return bits;
}

// One workgroup per image: min(D, G) rounds of "best covered gt, first box that covers it best" on the class-agnostic and the
// class-aware IoU matrices, each round recorded against the round index; hits and gt counts are integer atomics.
template <class Box>
__global__ __launch_bounds__(AR_THREADS) void proposal_ar_kernel(const int* __restrict__ gt_off, const float* __restrict__ gt_box,
                                                                 const int* __restrict__ gt_cls, const float* __restrict__ gt_ratio,
                                                                 const int* __restrict__ dt_off, const long long* __restrict__ dt_order,
                                                                 const float* __restrict__ dt_box, const int* __restrict__ dt_cls, int limit,
                                                                 int K1, int T, int R, int A, ArParams p,
                                                                 const long long* __restrict__ scratch_off, float* __restrict__ scratch,
                                                                 int* __restrict__ hits, int* __restrict__ counts) {
  constexpr int W = Box::W;
  constexpr int STAGE = Box::STAGE_LANES;
  static_assert(STAGE > 0 && STAGE <= AR_THREADS && STAGE % 64 == 0, "whole waves stage the matrices");
  __shared__ float s_ov[2 * AR_LDS_IOU];
  __shared__ float red_v[2][AR_THREADS];
  __shared__ int red_g[2][AR_THREADS], red_d[2][AR_THREADS];
  typename Box::Lds* lds = nullptr;
  if constexpr (Box::LDS_PER_LANE > 0) {
    __shared__ typename Box::Lds lane_lds[Box::LDS_PER_LANE * STAGE];
    lds = lane_lds + threadIdx.x;     // used by the staging lanes only
  }
  const int img = blockIdx.x;
  const int g0 = gt_off[img], G = gt_off[img + 1] - g0;
  const int d0 = dt_off[img];
  const int D = min(dt_off[img + 1] - d0, limit);
  if (G == 0 || D == 0) return;   // the image takes no part, its gts included
  const int RA = R * A;
  for (int g = threadIdx.x; g < G; g += AR_THREADS) {
    const int bits = ar_buckets(Box::area(gt_box + W * (size_t)(g0 + g)), gt_ratio[g0 + g], p, R, A);
    const int c = gt_cls[g0 + g];
    for (int r = 0; r < R; ++r)
      for (int a = 0; a < A; ++a)
        if (((bits >> r) & 1) && ((bits >> (8 + a)) & 1)) {
          atomicAdd(counts + (size_t)c * RA + r * A + a, 1);
          atomicAdd(counts + (size_t)(K1 - 1) * RA + r * A + a, 1);
        }
  }
  const size_t DG = (size_t)D * G;
  float* ov = DG <= AR_LDS_IOU ? s_ov : scratch + scratch_off[img];
  float* ovm = DG <= AR_LDS_IOU ? s_ov + AR_LDS_IOU : scratch + scratch_off[img] + (size_t)limit * G;
  if (STAGE == AR_THREADS || threadIdx.x < STAGE) {
    for (size_t idx = threadIdx.x; idx < DG; idx += STAGE) {
      const int d = (int)(idx / G), g = (int)(idx - (size_t)d * G);
      const long long q = dt_order[d0 + d];
      const float v = Box::overlap(dt_box + W * q, gt_box + W * (size_t)(g0 + g), lds);
      ov[idx] = v;
      ovm[idx] = v * (float)(dt_cls[q] == gt_cls[g0 + g]);
    }
  }
  __syncthreads();
  const int rounds = min(D, G);
  for (int j = 0; j < rounds; ++j) {
    // per column: the maximum over the boxes and the first box at it; then the first column at the maximum
    float bv[2] = {-INFINITY, -INFINITY};
    int bg[2] = {0x7fffffff, 0x7fffffff}, bd[2] = {0, 0};
    for (int g = threadIdx.x; g < G; g += AR_THREADS) {
      for (int w = 0; w < 2; ++w) {
        const float* M_ = w ? ovm : ov;
        float mv = M_[g];
        int md = 0;
        for (int d = 1; d < D; ++d) {
          const float v = M_[(size_t)d * G + g];
          if (v > mv) { mv = v; md = d; }
        }
        if (mv > bv[w]) { bv[w] = mv; bg[w] = g; bd[w] = md; }   // g ascending within a thread: first column kept on ties
      }
    }
    for (int w = 0; w < 2; ++w) {
      red_v[w][threadIdx.x] = bv[w];
      red_g[w][threadIdx.x] = bg[w];
      red_d[w][threadIdx.x] = bd[w];
    }
    __syncthreads();
    for (int o = AR_THREADS / 2; o > 0; o >>= 1) {
      if (threadIdx.x < o) {
        for (int w = 0; w < 2; ++w) {
          const float v2 = red_v[w][threadIdx.x + o];
          const int g2 = red_g[w][threadIdx.x + o];
          if (v2 > red_v[w][threadIdx.x] || (v2 == red_v[w][threadIdx.x] && g2 < red_g[w][threadIdx.x])) {
            red_v[w][threadIdx.x] = v2;
            red_g[w][threadIdx.x] = g2;
            red_d[w][threadIdx.x] = red_d[w][threadIdx.x + o];
          }
        }
      }
      __syncthreads();
    }
    const float best = red_v[0][0], best_m = red_v[1][0];
    const int gi = red_g[0][0], di = red_d[0][0], gi_m = red_g[1][0], di_m = red_d[1][0];
    __syncthreads();
    if (gi >= G || gi_m >= G) break;   // only NaN overlaps leave no winner (block-uniform: every thread read the same LDS words)
    // the round is recorded in the ratio / area buckets of the class-aware winner, for its class and for "all classes"
    if (threadIdx.x < T) {
      const int bits = ar_buckets(Box::area(gt_box + W * (size_t)(g0 + gi_m)), gt_ratio[g0 + gi_m], p, R, A);
      const int c = gt_cls[g0 + gi_m];
      const float th = p.thr[threadIdx.x];
      const bool h_m = best_m >= th, h = best >= th;
      for (int r = 0; r < R; ++r)
        for (int a = 0; a < A; ++a)
          if (((bits >> r) & 1) && ((bits >> (8 + a)) & 1)) {
            if (h_m) atomicAdd(hits + (((size_t)threadIdx.x * K1 + c) * R + r) * A + a, 1);
            if (h) atomicAdd(hits + (((size_t)threadIdx.x * K1 + (K1 - 1)) * R + r) * A + a, 1);
          }
    }
    for (int g = threadIdx.x; g < G; g += AR_THREADS) {
      ov[(size_t)di * G + g] = -1.f;
      ovm[(size_t)di_m * G + g] = -1.f;
    }
    for (int d = threadIdx.x; d < D; d += AR_THREADS) {
      ov[(size_t)d * G + gi] = -1.f;
      ovm[(size_t)d * G + gi_m] = -1.f;
    }
    __syncthreads();
  }
}

__global__ void proposal_ar_finalize(const int* __restrict__ hits, const int* __restrict__ counts, int n_per_t, int T,
                                     float* __restrict__ recalls) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_per_t * T) return;
  recalls[i] = (float)hits[i] / fmaxf((float)counts[i % n_per_t], 1.f);
}

// floats of an image's scratch slot: both [limit, G] matrices, where one of them outgrows its LDS half
inline long long proposal_ar_scratch_floats(int num_gts, int limit) {
  if (num_gts < 0 || limit < 0) return -1;
  if ((long long)num_gts * limit <= AR_LDS_IOU) return 0;
  return 2LL * limit * num_gts;
}

template <class Box>
int launch_proposal_ar(const int* gt_off, const float* gt_box, const int* gt_cls, const float* gt_ratio, const int* dt_off,
                       const long long* dt_order, const float* dt_box, const int* dt_cls, int num_img, int limit, int K1, const float* thr,
                       int T, const float* ratio_rng, int R, const float* area_rng, int A, const long long* scratch_off, float* scratch,
                       int* hits, int* counts, float* recalls, void* stream) {
  if (num_img < 0 || limit <= 0 || K1 <= 0 || T <= 0 || R <= 0 || A <= 0 || T > AR_MAX_T || R > AR_MAX_A || A > AR_MAX_A ||
      !thr || !ratio_rng || !area_rng || !hits || !counts || !recalls || (num_img > 0 && (!gt_off || !dt_off || !scratch_off)))
    return SOD_EARG;
  hipStream_t st = (hipStream_t)stream;
  ArParams p;
  for (int t = 0; t < T; ++t) p.thr[t] = thr[t];
  for (int r = 0; r < R; ++r) {
    p.rlo[r] = ratio_rng[2 * r];
    p.rhi[r] = ratio_rng[2 * r + 1];
  }
  for (int a = 0; a < A; ++a) {
    p.alo[a] = area_rng[2 * a];
    p.ahi[a] = area_rng[2 * a + 1];
  }
  if (num_img > 0)
    SOD_LAUNCH(proposal_ar_kernel<Box>, dim3(num_img), dim3(AR_THREADS), 0, st, gt_off, gt_box, gt_cls, gt_ratio, dt_off, dt_order, dt_box,
               dt_cls, limit, K1, T, R, A, p, scratch_off, scratch, hits, counts);
  const int n_per_t = K1 * R * A;
  SOD_LAUNCH(proposal_ar_finalize, dim3((n_per_t * T + 255) / 256), dim3(256), 0, st, hits, counts, n_per_t, T, recalls);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
