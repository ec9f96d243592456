// RotatedRetinaNet (modeling/meta_arch/rotated_retinanet.py): detectron2's rotated pieces in RetinaNet's slots - the intent of the
// reference's slender_det/modeling/meta_arch/retina/retina_rotated.py (Box2BoxTransformRotated at :71, RotatedBoxes.cat at :271), which
// still matches with the axis-aligned pairwise_iou and keeps a 4-wide head.
//   * sod_retina_label_rotated: pairwise_iou_rotated + Matcher + class mapping + Box2BoxTransformRotated.get_deltas of the WHOLE batch in
//     two launches (image = grid.y, the image's gt count read on the device).  Decision-identical to sod_anchor_match_rotated ->
//     sod_retina_targets' mapping -> sod_box2box_get_deltas per image: the same iou_rotated_lds, the same 64-bit "first maximum wins".
//     sod_retina_label_rotated_boxes: the same kernels writing the matched gt box itself instead of the deltas (the rotated IoU loss).
//   * sod_retina_decode_rotated: Box2BoxTransformRotated.apply_deltas on the candidates of sod_dense_topk_select, one launch per batch.
// Latency / HBM-bound fp32 work, no MFMA; the clipping's candidate points live in LDS (rotated_iou.h).
#include "common.h"
#include "../../include/slender_hip.h"
#include <math.h>

namespace {

#include "rotated_iou.h"
#include "box_transform.h"

constexpr int RR_GS = 8;                  // boxes per round of the labeller: at most 256 * RR_GS candidate pairs
constexpr int RR_MAX_LEVELS = 8;

struct LabelArgs {
  const float* anchors;      // (R, 5)
  const float* gts;          // (N, Gmax, 5)
  const int* classes;        // (N, Gmax)
  const int* counts;         // (N), on the device
  int R, Gmax;
  float lo, hi;
  int l0, l1, l2, low_quality, num_classes;
  W5 w;
  int* labels;               // (N, R)
  float* deltas;             // (N, R, 5): the deltas, or the matched gt boxes (retina_label1_rot_kernel<true>)
  unsigned* gt_best;         // (N, Gmax) IoU bits, zeroed by the call
};

__device__ __forceinline__ int class_of(int ml, int num_classes, const int* cls, int idx) {
  return (ml == 0) ? num_classes : ((ml == -1) ? -1 : cls[idx]);
}

// Circle test of every (anchor, box) pair of the round, survivors compacted into ``pairs`` (the two early returns of iou_rotated: a pair
// dropped here has IoU exactly 0 there).  Every thread of the workgroup calls it; returns the number of survivors.
__device__ __forceinline__ int compact_round(const float* a, float ra, bool live, const float* gts, int g0, int G, unsigned* pairs, int* npairs) {
  const int tid = threadIdx.x;
  if (tid == 0) *npairs = 0;
  __syncthreads();
  if (live) {
    const int g1 = min(G, g0 + RR_GS);
    for (int g = g0; g < g1; ++g) {
      const float* b = gts + g * 5;
      const float dx = b[0] - a[0], dy = b[1] - a[1], rs = ra + 0.5f * sqrtf(b[2] * b[2] + b[3] * b[3]);
      if (b[2] * b[3] >= 1e-14f && dx * dx + dy * dy <= rs * rs * 1.0001f) pairs[atomicAdd(npairs, 1)] = ((unsigned)tid << 16) | (unsigned)(g - g0);
    }
  }
  __syncthreads();
  return *npairs;
}

// Pass 1 (anchor_match1_rot_kernel of detection_ops.hip per image + the targets): per-anchor best IoU / matched box in LDS words and
// registers only, per-box best over all anchors into gt_best.  Writes the deltas (they depend on the match alone) and either the final
// label or, when pass 2 follows for the image, the match packed with the threshold label: (match << 2) | (label + 1).
// BOXES: the matched gt box instead of its deltas (zeros for an image without gts, as the deltas).
template <bool BOXES>
__global__ __launch_bounds__(256) void retina_label1_rot_kernel(const LabelArgs a) {
  extern __shared__ unsigned lbest[];   // [Gmax]
  __shared__ unsigned pairs[256 * RR_GS];
  __shared__ P2 rot_pts[24 * 256];      // 48 KB: the clipping's candidate points (see RotPtsLds)
  __shared__ unsigned long long abest[256];
  __shared__ int npairs;
  const int tid = threadIdx.x, n = blockIdx.y;
  const int G = min(max(a.counts[n], 0), a.Gmax);
  const float* gts = a.gts + (long long)n * a.Gmax * 5;
  const int* cls = a.classes + (long long)n * a.Gmax;
  int* labels = a.labels + (long long)n * a.R;
  float* deltas = a.deltas + (long long)n * a.R * 5;
  for (int g = tid; g < G; g += 256) lbest[g] = 0u;
  const int chunks = (a.R + 255) / 256;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int i = ch * 256 + tid;
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < a.R) {
#pragma unroll
      for (int e = 0; e < 5; ++e) s[e] = a.anchors[(long long)i * 5 + e];
    }
    const float ra = 0.5f * sqrtf(s[2] * s[2] + s[3] * s[3]);
    const bool live = i < a.R && s[2] * s[3] >= 1e-14f;
    abest[tid] = 0x00000000FFFFFFFFull;          // IoU 0 with box 0: what "v > bv" from bv = -1 leaves when every IoU is 0
    for (int g0 = 0; g0 < G; g0 += RR_GS) {
      const int np = compact_round(s, ra, live, gts, g0, G, pairs, &npairs);
      for (int t = tid; t < np; t += 256) {
        const unsigned pr = pairs[t];
        const int la = (int)(pr >> 16), g = g0 + (int)(pr & 0xffffu);
        float aa[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) aa[e] = a.anchors[((long long)ch * 256 + la) * 5 + e];
        const float v = fmaxf(iou_rotated_lds(gts + g * 5, aa, rot_pts + tid, 256), 0.f);
        if (v > 0.f) {
          atomicMax(&abest[la], ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)g));
          atomicMax(&lbest[g], __float_as_uint(v));
        }
      }
      __syncthreads();
    }
    if (i < a.R) {
      int lab = a.num_classes;
      float d[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (G > 0) {
        const unsigned long long bb = abest[tid];
        const float v = __uint_as_float((unsigned)(bb >> 32));
        const int m = (int)(0xFFFFFFFFu - (unsigned)(bb & 0xFFFFFFFFull));
        const int ml = (v < a.lo) ? a.l0 : ((v < a.hi) ? a.l1 : a.l2);
        lab = a.low_quality ? ((m << 2) | (ml + 1)) : class_of(ml, a.num_classes, cls, m);
        const float* t = gts + m * 5;
        if constexpr (BOXES) {
#pragma unroll
          for (int e = 0; e < 5; ++e) d[e] = t[e];
        } else {
          rot_get_deltas(s, t, a.w.w, d);
        }
      }
      labels[i] = lab;
#pragma unroll
      for (int e = 0; e < 5; ++e) deltas[(long long)i * 5 + e] = d[e];
    }
    __syncthreads();
  }
  __syncthreads();
  for (int g = tid; g < G; g += 256) atomicMax(&a.gt_best[(long long)n * a.Gmax + g], lbest[g]);
}

// Pass 2 (anchor_match2_kernel<5> per image + retina_targets_kernel's class mapping): low-quality promotion, `Q == best_per_gt[:, None]`.
// A box whose best IoU over all anchors is 0 equals the (zero) IoU of EVERY anchor: the whole image is promoted, as the per-image kernel
// does.  Otherwise only pairs that pass the circle test can attain a box's (positive) best: the same compaction as pass 1.
__global__ __launch_bounds__(256) void retina_label2_rot_kernel(const LabelArgs a) {
  extern __shared__ unsigned lbest[];   // [Gmax]
  __shared__ unsigned pairs[256 * RR_GS];
  __shared__ P2 rot_pts[24 * 256];
  __shared__ int promo[256];
  __shared__ int npairs;
  const int tid = threadIdx.x, n = blockIdx.y;
  const int G = min(max(a.counts[n], 0), a.Gmax);
  if (G == 0) return;                   // pass 1 wrote the final labels of an image without boxes (uniform over the workgroup)
  const float* gts = a.gts + (long long)n * a.Gmax * 5;
  const int* cls = a.classes + (long long)n * a.Gmax;
  int* labels = a.labels + (long long)n * a.R;
  int zero = 0;
  for (int g = tid; g < G; g += 256) {
    const unsigned b = a.gt_best[(long long)n * a.Gmax + g];
    lbest[g] = b;
    zero |= (b == 0u);
  }
  const int all = __syncthreads_or(zero);
  const int chunks = (a.R + 255) / 256;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int i = ch * 256 + tid;
    promo[tid] = all;
    if (!all) {
      float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (i < a.R) {
#pragma unroll
        for (int e = 0; e < 5; ++e) s[e] = a.anchors[(long long)i * 5 + e];
      }
      const float ra = 0.5f * sqrtf(s[2] * s[2] + s[3] * s[3]);
      const bool live = i < a.R && s[2] * s[3] >= 1e-14f;
      for (int g0 = 0; g0 < G; g0 += RR_GS) {
        const int np = compact_round(s, ra, live, gts, g0, G, pairs, &npairs);
        for (int t = tid; t < np; t += 256) {
          const unsigned pr = pairs[t];
          const int la = (int)(pr >> 16), g = g0 + (int)(pr & 0xffffu);
          float aa[5];
#pragma unroll
          for (int e = 0; e < 5; ++e) aa[e] = a.anchors[((long long)ch * 256 + la) * 5 + e];
          const float v = fmaxf(iou_rotated_lds(gts + g * 5, aa, rot_pts + tid, 256), 0.f);
          if (v == __uint_as_float(lbest[g])) promo[la] = 1;
        }
        __syncthreads();
      }
    }
    if (i < a.R) {
      const int pk = labels[i];
      const int ml = promo[tid] ? 1 : (pk & 3) - 1;
      labels[i] = class_of(ml, a.num_classes, cls, pk >> 2);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- decode
struct DecodeArgs {
  const float* pred;        // (N, P, pitch)
  const float* anchors;     // (P * A, 5)
  const int* rows;          // (N, M) row inside the slot's level
  const float* scores;      // (N, M), -inf = empty slot
  int N, P, A, pitch, M, top_n;
  int row0[RR_MAX_LEVELS];  // first anchor of each level
  W5 w;
  float clampv;
  float* out;               // (N, M, 5)
};

__global__ __launch_bounds__(256) void retina_decode_rot_kernel(const DecodeArgs a) {
  const long long total = (long long)a.N * a.M, R = (long long)a.P * a.A;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long n = i / a.M;
    const int m = (int)(i - n * a.M);
    float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const long long r = (long long)a.rows[i] + a.row0[m / a.top_n];
    if (a.scores[i] != -__builtin_inff() && r >= 0 && r < R) {
      const long long px = r / a.A;
      const int an = (int)(r - px * a.A);
      const float* d = a.pred + (n * a.P + px) * a.pitch + an * 5;
      const float* b = a.anchors + r * 5;
      rot_apply_deltas(d, b, a.w.w, a.clampv, o);      // a NaN dw / dh is clamped away, any other NaN zeroes the box
      if (!(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(o[3]) && isfinite(o[4]))) {
#pragma unroll
        for (int e = 0; e < 5; ++e) o[e] = 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 5; ++e) a.out[i * 5 + e] = o[e];
  }
}

inline bool matcher_label(int l) { return l >= -1 && l <= 1; }

}  // namespace

template <bool BOXES>
static int label_rotated(const float* anchors, int R, const float* gt_boxes, const int* gt_classes, const int* gt_counts, int N,
                         int Gmax, float thr_lo, float thr_hi, int label_below, int label_between, int label_above,
                         int allow_low_quality, int num_classes, const float* weights5, int* gt_labels, float* gt_deltas,
                         unsigned* gt_best_ws, void* stream) {
  LabelArgs a{};
  if (!anchors || R <= 0 || !gt_counts || N <= 0 || N > 65535 || Gmax < 0 || Gmax > SOD_RETINA_LABEL_MAX_GT || num_classes <= 0 || !gt_labels || !gt_deltas ||
      !fill_w5(a.w, weights5) || !matcher_label(label_below) || !matcher_label(label_between) || !matcher_label(label_above))
    return SOD_EARG;
  if (Gmax > 0 && (!gt_boxes || !gt_classes || !gt_best_ws)) return SOD_EARG;
  if ((long long)R * 5 > 0x7fffffffLL) return SOD_ESIZE;
  hipStream_t st = (hipStream_t)stream;
  if (Gmax > 0) {
    hipError_t e = hipMemsetAsync(gt_best_ws, 0, sizeof(unsigned) * (size_t)N * Gmax, st);
    if (e != hipSuccess) return (int)e;
  }
  a.anchors = anchors; a.gts = gt_boxes; a.classes = gt_classes; a.counts = gt_counts; a.R = R; a.Gmax = Gmax;
  a.lo = thr_lo; a.hi = thr_hi; a.l0 = label_below; a.l1 = label_between; a.l2 = label_above;
  a.low_quality = (allow_low_quality && Gmax > 0) ? 1 : 0;
  a.num_classes = num_classes; a.labels = gt_labels; a.deltas = gt_deltas; a.gt_best = gt_best_ws;
  const dim3 grid(sod_nblk(R, 2048), N);
  const size_t lds = sizeof(unsigned) * (Gmax > 0 ? Gmax : 1);
  SOD_LAUNCH(retina_label1_rot_kernel<BOXES>, grid, dim3(256), lds, st, a);
  if (a.low_quality) SOD_LAUNCH(retina_label2_rot_kernel, grid, dim3(256), lds, st, a);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}

extern "C" int sod_retina_label_rotated(const float* anchors, int R, const float* gt_boxes, const int* gt_classes, const int* gt_counts, int N,
                                        int Gmax, float thr_lo, float thr_hi, int label_below, int label_between, int label_above,
                                        int allow_low_quality, int num_classes, const float* weights5, int* gt_labels, float* gt_deltas,
                                        unsigned* gt_best_ws, void* stream) {
  return label_rotated<false>(anchors, R, gt_boxes, gt_classes, gt_counts, N, Gmax, thr_lo, thr_hi, label_below, label_between, label_above,
                              allow_low_quality, num_classes, weights5, gt_labels, gt_deltas, gt_best_ws, stream);
}

extern "C" int sod_retina_label_rotated_boxes(const float* anchors, int R, const float* gt_boxes, const int* gt_classes, const int* gt_counts,
                                              int N, int Gmax, float thr_lo, float thr_hi, int label_below, int label_between, int label_above,
                                              int allow_low_quality, int num_classes, const float* weights5, int* gt_labels,
                                              float* matched_boxes, unsigned* gt_best_ws, void* stream) {
  return label_rotated<true>(anchors, R, gt_boxes, gt_classes, gt_counts, N, Gmax, thr_lo, thr_hi, label_below, label_between, label_above,
                             allow_low_quality, num_classes, weights5, gt_labels, matched_boxes, gt_best_ws, stream);
}

extern "C" int sod_retina_decode_rotated(const float* pred, int pitch, const float* anchors, const int* rows, const float* scores, int N, int P,
                                         int A, int M, int top_n, const int* level_row0, int nlev, const float* weights5, float scale_clamp,
                                         float* out, void* stream) {
  DecodeArgs a{};
  if (!pred || !anchors || !rows || !scores || !out || !level_row0 || N <= 0 || P <= 0 || A <= 0 || pitch < A * 5 || M < 0 || top_n <= 0 ||
      nlev <= 0 || nlev > RR_MAX_LEVELS || M != nlev * top_n || !fill_w5(a.w, weights5))
    return SOD_EARG;
  if (M == 0) return SOD_OK;
  for (int l = 0; l < nlev; ++l) {
    if (level_row0[l] < 0 || (long long)level_row0[l] > (long long)P * A) return SOD_EARG;
    a.row0[l] = level_row0[l];
  }
  a.pred = pred; a.anchors = anchors; a.rows = rows; a.scores = scores; a.N = N; a.P = P; a.A = A; a.pitch = pitch; a.M = M; a.top_n = top_n;
  a.clampv = scale_clamp; a.out = out;
  SOD_LAUNCH(retina_decode_rot_kernel, dim3(sod_nblk((long long)N * M, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  SOD_CHECK_LAUNCH();
  return SOD_OK;
}
